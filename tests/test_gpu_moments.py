"""Posterior moments on the device: the reduction kernel against a sequential fp64 loop on the host (bitwise), and the trainer's
`mcpc_moments` against the recorded trajectory of the same call."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the kernel ------------------------------------------------------------------------------------------------
def _host_sums(rec, rows, s0=None, q0=None):
    """The definition: a sequential fp64 loop over the records, in ascending order."""
    s = np.zeros(rec.shape[1], np.float64) if s0 is None else s0.copy()
    q = np.zeros(rec.shape[1], np.float64) if q0 is None else q0.copy()
    for r in rows:
        v = rec[r].astype(np.float64)
        s = s + v
        q = q + v * v
    return s, q


def _records(n_rec, row, seed, offset=0, special=False):
    """[n_rec, row] fp32 on the device, `offset` floats into its allocation; values 3 N(0,1) + 1.5."""
    g = torch.Generator().manual_seed(seed)
    host = 3.0 * torch.randn(n_rec, row, generator=g) + 1.5
    if special:
        vals = torch.tensor([3e38, -3e38, 1e-40, -1e-42, 1.17549435e-38, 0.0, -0.0, 1.5], dtype=torch.float32)
        host = vals[torch.randint(0, len(vals), (n_rec, row), generator=g)]
        assert (host.abs() < 1.17549435e-38).any() and (host.abs() > 1e38).any()
    alloc = torch.empty(n_rec * row + offset, dtype=torch.float32, device=DEV)
    rec = alloc[offset:].view(n_rec, row)
    rec.copy_(host)
    assert rec.is_contiguous() and rec.data_ptr() == alloc.data_ptr() + 4 * offset
    return rec, host.numpy()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def _assert_bitwise(got, want, what):
    assert np.array_equal(_bits(got), want.view(np.int64)), what


WINDOWS = [(0, 1, 1), (0, 1, 2), (3, 2, 7), (5, 7, 8), (0, 1, 37)]


@pytest.mark.parametrize("first, stride, n", WINDOWS)
@pytest.mark.parametrize("row, offset", [(1, 0), (15, 0), (15, 1), (1280, 0), (1280, 1), (2310, 0), (50176, 0)])
def test_kernel_is_the_sequential_fp64_loop(row, offset, first, stride, n):
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    n_rec = first + (n - 1) * stride + 3
    rec, host = _records(n_rec, row, seed=row + n, offset=offset)
    rows = [first + k * stride for k in range(n)]
    g = torch.Generator().manual_seed(1)
    s0 = torch.randn(row, generator=g, dtype=torch.float64) * 1e3
    q0 = torch.randn(row, generator=g, dtype=torch.float64).abs() * 1e5
    # accumulate = 0 onto garbage
    s, q = s0.to(DEV), q0.to(DEV)
    moments_accumulate(rec, first, stride, n, s, q, accumulate=False)
    ws, wq = _host_sums(host, rows)
    _assert_bitwise(s, ws, "sum, overwrite")
    _assert_bitwise(q, wq, "sumsq, overwrite")
    # accumulate = 1 onto known values
    s, q = s0.to(DEV), q0.to(DEV)
    moments_accumulate(rec, first, stride, n, s, q, accumulate=True)
    ws1, wq1 = _host_sums(host, rows, s0.numpy(), q0.numpy())
    _assert_bitwise(s, ws1, "sum, accumulate")
    _assert_bitwise(q, wq1, "sumsq, accumulate")
    # no sumsq
    s = s0.to(DEV)
    moments_accumulate(rec, first, stride, n, s, None, accumulate=False)
    _assert_bitwise(s, ws, "sum alone")


@pytest.mark.parametrize("row", [15, 1280])
def test_kernel_extreme_values_and_denormals(row):
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    rec, host = _records(12, row, seed=3, special=True)
    s = torch.empty(row, dtype=torch.float64, device=DEV)
    q = torch.empty(row, dtype=torch.float64, device=DEV)
    moments_accumulate(rec, 1, 2, 5, s, q, accumulate=False)
    ws, wq = _host_sums(host, [1, 3, 5, 7, 9])
    assert np.isfinite(wq).all() and wq.max() > 1e76
    _assert_bitwise(s, ws, "sum")
    _assert_bitwise(q, wq, "sumsq")


def test_kernel_n_zero():
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    rec, _ = _records(2, 16, seed=0)
    s = torch.full((16,), 7.0, dtype=torch.float64, device=DEV)
    q = torch.full((16,), 9.0, dtype=torch.float64, device=DEV)
    moments_accumulate(rec, 0, 1, 0, s, q, accumulate=True)
    assert (s == 7.0).all() and (q == 9.0).all()
    moments_accumulate(rec, 0, 1, 0, s, q, accumulate=False)
    assert (s == 0.0).all() and (q == 0.0).all()


@pytest.mark.parametrize("row, offset", [(2310, 0), (1280, 0), (1280, 1)])
def test_chunk_invariance(row, offset):
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    rec, host = _records(37, row, seed=11, offset=offset)
    one = [torch.empty(row, dtype=torch.float64, device=DEV) for _ in range(2)]
    moments_accumulate(rec, 0, 1, 37, one[0], one[1], accumulate=False)
    parts = [torch.zeros(row, dtype=torch.float64, device=DEV) for _ in range(2)]
    for first, n in ((0, 1), (1, 5), (6, 31)):
        moments_accumulate(rec, first, 1, n, parts[0], parts[1], accumulate=True)
    for a, b in zip(one, parts):
        assert np.array_equal(_bits(a), _bits(b))
    ws, wq = _host_sums(host, range(37))
    _assert_bitwise(parts[0], ws, "sum")
    _assert_bitwise(parts[1], wq, "sumsq")


def test_offsets_are_64_bit():
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    row = 1 << 20
    try:
        rec = torch.empty(2049, row, dtype=torch.float32, device=DEV)         # 8.6 GB; row 2048 starts at element 2^31
    except RuntimeError as exc:                                                # (torch.OutOfMemoryError is one)
        pytest.skip(f"no room for the 8.6 GB record buffer: {exc}")
    g = torch.Generator().manual_seed(4)
    host = {}
    for r in (2040, 2044, 2048):
        h = 3.0 * torch.randn(row, generator=g) + 1.5
        rec[r].copy_(h)
        host[r] = h.numpy()
    s = torch.empty(row, dtype=torch.float64, device=DEV)
    q = torch.empty(row, dtype=torch.float64, device=DEV)
    moments_accumulate(rec, 2040, 4, 3, s, q, accumulate=False)
    ws, wq = np.zeros(row), np.zeros(row)
    for r in (2040, 2044, 2048):
        v = host[r].astype(np.float64)
        ws = ws + v
        wq = wq + v * v
    _assert_bitwise(s, ws, "sum")
    _assert_bitwise(q, wq, "sumsq")
    del rec
    torch.cuda.empty_cache()


def test_sigmoid_transform():
    """sigmoid_f is one exp2, one add, one rcp and one multiply on values <= 1: at most about 8 half-ulps of 1.0 = 4.8e-7 per sample,
    twice that for its square.  The mean of 64 samples cannot be further off than one sample."""
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    g = torch.Generator().manual_seed(6)
    logits = (torch.rand(64, 2310, generator=g) * 60.0 - 30.0)
    rec = logits.to(DEV)
    s = torch.empty(2310, dtype=torch.float64, device=DEV)
    q = torch.empty(2310, dtype=torch.float64, device=DEV)
    moments_accumulate(rec, 0, 1, 64, s, q, transform="sigmoid", accumulate=False)
    ref = 1.0 / (1.0 + np.exp(-logits.numpy().astype(np.float64)))
    e1 = np.abs(s.cpu().numpy() / 64 - ref.mean(0)).max()
    e2 = np.abs(q.cpu().numpy() / 64 - (ref * ref).mean(0)).max()
    print(f"sigmoid moments: max |mean error| {e1:.3e} (bound 5e-7), max |mean-square error| {e2:.3e} (bound 1e-6)")
    assert e1 <= 5e-7 and e2 <= 1e-6, (e1, e2)


def test_einval_cases():
    from montecarlopredictivecoding_amd import _lib as L
    lib = L.load()
    rec = torch.zeros(4, 8, dtype=torch.float32, device=DEV)
    s = torch.zeros(8, dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    R, S = C.c_void_p(rec.data_ptr()), C.c_void_p(s.data_ptr())

    def call(rec_=R, row=8, first=0, stride=1, n=2, xf=0, sum_=S):
        code = lib.mcpc_moments_accumulate(0, rec_, row, first, stride, n, xf, sum_, None, 0, stream)
        return code, lib.mcpc_last_error().decode()

    assert call()[0] == 0
    for kw, word in ((dict(sum_=None), "sum is null"), (dict(rec_=None), "rec is null"), (dict(row=0), "row_elems=0"),
                     (dict(stride=0), "stride=0"), (dict(first=-1), "first=-1"), (dict(n=-1), "n=-1"),
                     (dict(xf=2), "unknown transform 2")):
        code, msg = call(**kw)
        assert code == -1 and word in msg, (kw, code, msg)
    assert call(rec_=None, n=0)[0] == 0                      # a null rec is fine when no record is read
    torch.cuda.synchronize()
    assert (s == 0).all()


def test_binding_checks_its_tensors():
    from montecarlopredictivecoding_amd.engine import moments_accumulate
    rec = torch.zeros(4, 8, dtype=torch.float32, device=DEV)
    s = torch.zeros(8, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="holds 4 records"):
        moments_accumulate(rec, 1, 2, 3, s)
    with pytest.raises(TypeError):
        moments_accumulate(rec, 0, 1, 2, s.float())
    with pytest.raises(ValueError, match="elements"):
        moments_accumulate(rec, 0, 1, 2, s[:7])
    with pytest.raises(ValueError, match="contiguous"):
        moments_accumulate(rec[:, ::2], 0, 1, 2, s[:4].clone())
    with pytest.raises(ValueError, match="device"):
        moments_accumulate(rec, 0, 1, 2, s.cpu())


# ---- the trainer -----------------------------------------------------------------------------------------------
SIZES, N_OUT, B, T = (6, 16, 16), 24, 40, 60
SPEC = dict(begin=20, stride=3, layers=(0, 2), outputs="identity")


def _net(device, loss="bernoulli"):
    """6-16-16 -> 24, ReLU; the same weights, data and x0 on whichever device."""
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


def _call(um, model, data, inputs, moments, chunk=None, every_t=True, update_p_at="never", records=True, **kw):
    import montecarlopredictivecoding_amd.predictive_coding as pc
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    tr = pc.PCTrainer(model, T=T, optimizer_x_fn=torch.optim.SGD, optimizer_x_kwargs={"lr": 0.05}, update_p_at=update_p_at,
                      accumulate_p_at=list(range(40, T)) if update_p_at == "last" else "never",
                      optimizer_p_fn=torch.optim.Adam, optimizer_p_kwargs={"lr": 0.01}, plot_progress_at=[])
    tr.mcpc_seed = 5
    tr.mcpc_moments = moments
    if chunk is not None:
        tr.mcpc_moments_chunk_bytes = chunk
    base = pt._PHILOX_STEPS[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tr.train_on_batch(inputs=inputs, loss_fn=um.bernoulli_fn, loss_fn_kwargs={"_target": data, "_var": None},
                                callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr}, is_log_progress=False,
                                is_return_results_every_t=every_t, is_return_xs=records, is_return_outputs=records, **kw)
    pt._PHILOX_STEPS[0] = base                               # the next run replays the same noise
    return tr, res


def _loop(tensors):
    s = np.zeros(tensors[0].shape, np.float64)
    q = np.zeros(tensors[0].shape, np.float64)
    for t in tensors:
        v = t.detach().cpu().numpy().astype(np.float64)
        s = s + v
        q = q + v * v
    return s, q


def _within_ulps(got, want64, ulps):
    want = want64.astype(np.float32)
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)).all())


def _check_one_call_gives_both(device):
    um, model, data, inputs = _net(device)
    tr, res = _call(um, model, data, inputs, SPEC)
    assert tr.last_call_mode == "fused"
    m = tr.mcpc_last_moments
    steps = list(range(20, T, 3))
    assert m.n == 14 == len(steps)
    assert len(res["xs"]) == T and len(res["outputs"]) == T
    for l in (0, 2):
        s, q = _loop([res["xs"][t][l] for t in steps])
        assert m.x_sum[l].device.type == torch.device(device).type and m.x_sum[l].dtype == torch.float64
        _assert_bitwise(m.x_sum[l], s, f"x_sum[{l}]")
        _assert_bitwise(m.x_sumsq[l], q, f"x_sumsq[{l}]")
        traj = np.stack([res["xs"][t][l].numpy().astype(np.float64) for t in steps])
        assert m.x_var[l].dtype == torch.float32
        assert _within_ulps(m.x_var[l].cpu().numpy(), traj.var(0, ddof=1), 2)
        assert _within_ulps(m.x_mean[l].cpu().numpy(), traj.mean(0), 1)
    s, q = _loop([res["outputs"][t] for t in steps])
    _assert_bitwise(m.out_sum, s, "out_sum")
    _assert_bitwise(m.out_sumsq, q, "out_sumsq")
    assert m.x_mean[1] is None and m.x_var[1] is None and m.x_sum[1] is None
    assert m.out_mean.shape == (B, N_OUT) and m.out_var.shape == (B, N_OUT)
    return m


def test_one_call_gives_trajectory_and_moments():
    _check_one_call_gives_both(DEV)


def _state(tr, model, res):
    xs = [x.detach().clone() for x in tr.get_model_xs()]
    lin = [p for m in model if isinstance(m, torch.nn.Linear) for p in m.parameters()]
    grads = [p.grad.clone() for p in lin]
    params = [p.detach().clone() for p in lin]
    return xs, grads, params, {k: res[k] for k in ("loss", "energy", "overall")}


def _same_moments(a, b):
    for p, q in ((a.out_sum, b.out_sum), (a.out_sumsq, b.out_sumsq), *zip(a.x_sum, b.x_sum), *zip(a.x_sumsq, b.x_sumsq)):
        assert (p is None) == (q is None)
        if p is not None:
            assert np.array_equal(_bits(p), _bits(q))
    assert a.n == b.n


@pytest.mark.parametrize("every_t", [True, False])
def test_nothing_else_moves(every_t):
    um, model, data, inputs = _net(DEV)
    w0 = {k: v.clone() for k, v in model.state_dict().items() if "_x" not in k}
    spec = dict(begin=20, stride=3, layers=(0, 2), outputs="sigmoid")
    step_bytes = 4 * B * (SIZES[0] + SIZES[2] + N_OUT)
    runs = []
    for moments, chunk in ((None, None), (spec, None), (spec, 10 * step_bytes)):
        model.load_state_dict(w0, strict=False)
        for p in model.parameters():
            p.grad = None
        # (not every_t: the caller's own last-step records ride on the moments' ring)
        tr, res = _call(um, model, data, inputs, moments, chunk=chunk, every_t=every_t, update_p_at="last", records=not every_t)
        assert tr.last_call_mode == "fused"
        runs.append((tr, res, _state(tr, model, res)))
    # (slices of at most 10 steps; the 20 steps that accumulate parameter gradients stay one slice: a cut there would regroup their fp32 sums)
    assert [r[0].last_record_slices for r in runs[:2]] == [0, 1] and runs[2][0].last_record_slices >= 5
    assert runs[0][0].mcpc_last_moments is None
    xs0, g0, p0, e0 = runs[0][2]
    assert len(g0) == len(p0) == 8 and len(e0["overall"]) == (T if every_t else 1)
    for _, res, (xs, g, p, e) in runs[1:]:
        assert e == e0
        for a, b in zip(xs0 + g0 + p0, xs + g + p):
            assert torch.equal(a, b)
        if not every_t:
            assert len(res["outputs"]) == 1 and len(res["xs"]) == 1
            assert torch.equal(res["outputs"][0], runs[0][1]["outputs"][0])
            for a, b in zip(res["xs"][0], runs[0][1]["xs"][0]):
                assert torch.equal(a, b)
    _same_moments(runs[1][0].mcpc_last_moments, runs[2][0].mcpc_last_moments)
    assert runs[1][0].mcpc_last_moments.n == 14


def test_moments_do_not_depend_on_every_t_or_variance():
    um, model, data, inputs = _net(DEV)
    a = _call(um, model, data, inputs, SPEC, records=False, every_t=True)[0].mcpc_last_moments
    b = _call(um, model, data, inputs, SPEC, records=False, every_t=False)[0].mcpc_last_moments
    _same_moments(a, b)
    c = _call(um, model, data, inputs, dict(SPEC, variance=False), records=False, every_t=False)[0].mcpc_last_moments
    assert c.out_sumsq is None and c.x_sumsq[0] is None and c.out_var is None and c.x_var[0] is None
    assert np.array_equal(_bits(c.out_sum), _bits(a.out_sum)) and np.array_equal(_bits(c.x_sum[2]), _bits(a.x_sum[2]))
    one = _call(um, model, data, inputs, dict(begin=T - 1, layers=(0,)), records=False, every_t=False)[0].mcpc_last_moments
    assert one.n == 1 and torch.isnan(one.x_var[0]).all() and torch.isfinite(one.x_mean[0]).all()


def test_layer_wise_kernels(monkeypatch):
    monkeypatch.setenv("MCPC_TUNING", "ws=4")
    _check_one_call_gives_both(DEV)


def test_cpu_built_model():
    m_dev = _check_one_call_gives_both(DEV)
    m_cpu = _check_one_call_gives_both("cpu")
    for t in (m_cpu.out_sum, m_cpu.x_sum[0], m_cpu.x_sumsq[2], m_cpu.out_mean, m_cpu.x_var[0]):
        assert t.device.type == "cpu"
    _same_moments(m_cpu, m_dev)


def test_calls_that_are_not_fused_are_rejected():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    um, model, data, inputs = _net(DEV)
    x_before = [None if x is None else x.detach().clone() for x in (m.get_x() for m in model if hasattr(m, "get_x"))]
    with pytest.raises(NotImplementedError, match="step by step.*update_p_at"):
        _call(um, model, data, inputs, dict(layers=(0,)), update_p_at="all")
    assert all(x is None for x in x_before) and all(m.get_x() is None for m in model if hasattr(m, "get_x"))   # before any work
    tr, res = _call(um, model, data, inputs, None, update_p_at="all", records=False)
    assert tr.last_call_mode == "stepwise" and len(res["overall"]) == T
    masked = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(M=torch.ones(3, device=DEV)), torch.nn.Linear(3, 2)).to(DEV)
    masked.train()
    tr = pc.PCTrainer(masked, T=3, update_p_at="never", plot_progress_at=[])
    tr.mcpc_moments = dict(layers=(0,))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="generic torch loop.*S/M masks"):
            tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
        tr.mcpc_moments = None
        res = tr.train_on_batch(inputs=torch.zeros(2, 3, device=DEV), is_log_progress=False, is_return_results_every_t=False)
    assert tr.last_call_mode == "generic" and len(res["overall"]) == 1
    # a bad request on a call that would be fused: ValueError, before any work
    with pytest.raises(ValueError, match="layer index"):
        _call(um, model, data, inputs, dict(layers=(3,)))
    with pytest.raises(ValueError, match="begin"):
        _call(um, model, data, inputs, dict(begin=T))


# ---- the helpers -----------------------------------------------------------------------------------------------
def _helper_setup(loss):
    import montecarlopredictivecoding_amd.utils.model as um
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_mcpc_trainer, get_pc_trainer
    torch.manual_seed(5)
    cfg = dict(input_size=SIZES[0], hidden_size=SIZES[1], hidden2_size=SIZES[2], output_size=N_OUT, activation_fn="relu",
               loss_fn=um.bernoulli_fn if loss == "bernoulli" else um.fe_fn, input_var=0.3,
               T_pc=40, optimizer_x_fn_pc=torch.optim.Adam, optimizer_x_kwargs_pc={"lr": 0.1},
               mixing=20, sampling=40, optimizer_x_kwargs_mcpc={"lr": 0.03},
               optimizer_p_fn_mcpc=torch.optim.Adam, optimizer_p_kwargs_mcpc={"lr": 0.01})
    model = um.get_model(cfg, True, sample_x_fn=um.sample_x_fn_normal)
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(32, N_OUT, generator=g) < 0.3).float()
    loader = DataLoader(TensorDataset(data, torch.arange(32) % 10), batch_size=16)
    return um, cfg, model, loader, get_pc_trainer, get_mcpc_trainer


def test_get_posterior_expectation():
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    um, cfg, model, loader, get_pc_trainer, get_mcpc_trainer = _helper_setup("bernoulli")
    trainers = [get_pc_trainer(model, cfg, is_mcpc=True, training=False), get_mcpc_trainer(model, cfg, training=False)]
    base = pt._PHILOX_STEPS[0]
    recorded = []
    orig = trainers[1].train_on_batch

    def spy(*a, **kw):                                       # keep the trajectories get_representations reduces
        r = orig(*a, **kw)
        if "representations" in r:
            recorded.append(torch.stack(r["representations"]).numpy().astype(np.float64))
        return r
    trainers[1].train_on_batch = spy
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        ds_ref = um.get_representations(model, cfg, trainers, loader, rep_type="expectation", use_cuda=True)
        pt._PHILOX_STEPS[0] = base
        torch.manual_seed(7)
        ds = um.get_posterior_expectation(model, cfg, trainers, loader, use_cuda=True)
        pt._PHILOX_STEPS[0] = base
        torch.manual_seed(7)
        ds_v = um.get_posterior_expectation(model, cfg, trainers, loader, use_cuda=True, with_variance=True)
    assert trainers[1].mcpc_moments is None and len(recorded) == 2
    traj = np.concatenate(recorded, axis=1)                  # [T, 32, n_1]
    Tm = cfg["mixing"] + cfg["sampling"]
    assert traj.shape == (Tm, 32, SIZES[0])
    assert len(ds.tensors) == 2 and len(ds_v.tensors) == 3
    assert ds.tensors[0].shape == ds_ref.tensors[0].shape == (32, SIZES[0]) and ds.tensors[0].dtype == torch.float32
    assert torch.equal(ds.tensors[1].cpu(), ds_ref.tensors[1].cpu()) and torch.equal(ds.tensors[0], ds_v.tensors[0])
    bound = Tm * 2.0 ** -24 * np.abs(traj).max()             # the worst case of torch's fp32 mean over T terms
    err = (ds.tensors[0] - ds_ref.tensors[0]).abs().max().item()
    print(f"posterior expectation against get_representations: max |difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert _within_ulps(ds.tensors[0].cpu().numpy(), traj.mean(0), 1)
    assert ds_v.tensors[2].shape == (32, SIZES[0])
    assert _within_ulps(ds_v.tensors[2].cpu().numpy(), traj.var(0, ddof=1), 2)


@pytest.mark.parametrize("loss", ["bernoulli", "gaussian"])
def test_get_mse_rec_posterior(loss):
    import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
    from montecarlopredictivecoding_amd.utils.training_evaluation import get_mse_rec_posterior
    um, cfg, model, loader, get_pc_trainer, get_mcpc_trainer = _helper_setup(loss)
    base = pt._PHILOX_STEPS[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(7)
        got = get_mse_rec_posterior(model, cfg, loader, True)
        pt._PHILOX_STEPS[0] = base
        torch.manual_seed(7)
        # the same protocol from a recorded trajectory
        loss_fn = um.bernoulli_fn_mask if loss == "bernoulli" else um.fe_fn_mask
        pc_tr = get_pc_trainer(model, cfg, is_mcpc=True, training=False)
        mc_tr = get_mcpc_trainer(model, cfg, training=False)
        mse, count = 0.0, 0
        for data, _ in loader:
            data = data.to(DEV)
            kw = dict(inputs=torch.zeros(data.shape[0], SIZES[0], device=DEV), loss_fn=loss_fn,
                      loss_fn_kwargs={"_target": data, "_var": cfg["input_var"]}, is_log_progress=False,
                      is_checking_after_callback_after_t=False)
            pc_tr.train_on_batch(is_return_results_every_t=False, **kw)
            r = mc_tr.train_on_batch(callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": mc_tr},
                                     is_sample_x_at_batch_start=False, is_return_results_every_t=True, is_return_outputs=True, **kw)
            outs = torch.stack(r["outputs"][cfg["mixing"]:]).double()
            img = outs.sigmoid().mean(0) if loss == "bernoulli" else outs.mean(0)
            if loss == "bernoulli":
                img = (img > 0.5).double()
            half = round(data.shape[1] / 2)
            mse += float(((img[:, :-half] - data[:, :-half].double()) ** 2).mean(1).sum())
            count += data.shape[0]
    want = mse / count
    print(f"get_mse_rec_posterior ({loss}): {got:.9g}, from the trajectory {want:.9g}")
    assert mc_tr.last_call_mode == "fused"
    assert abs(got - want) <= 1e-6 * abs(want)

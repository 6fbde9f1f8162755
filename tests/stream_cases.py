"""Every entry point of include/mcpc.h that takes a stream, run on a SIDE stream whose inputs are still pending.

The library promises "all launches are asynchronous on the given stream" and the binding "on the current torch stream".  A suite that
only ever has torch's default stream current cannot tell a launch, a zero-fill or a finish kernel that went to stream 0 from one that
went where it was told.  This module holds the one scenario that can, and the table of cases it is run on (tests/test_gpu_streams.py
runs them on the device, tests/test_stream_cases.py checks the table against the header without one).

THE SCENARIO (`run_scenario`).  A case supplies its inputs (`inputs`, NumPy, no device needed), which of them are `pending`, the
initial contents of its outputs and accumulators (`outputs`: a sentinel for an overwriting call, the prior state for an accumulating
one), what it does before the delay (`before`: engines, binds, one warm-up call on data of its own), and the call under test (`call`).
 1. On the default stream, synchronised, the sequence below runs once without a delay; the clones of its outputs are `want`.  The
    suite holds these default-stream results to their fp64 references elsewhere: `want` is the anchor, not a new reference.
 2. Fresh input buffers hold poison: NaN for float data; for a tensor the kernel uses as an index, a count or a bit pattern
    (`Case.index`) a valid value that differs from the real one, so that no launch reads out of bounds whichever stream it lands on.
    Outputs and accumulators are allocated too.  torch.cuda.synchronize().
 3. With a torch.cuda.Stream() `s` current (`side_stream`: one that does not share a hardware queue with the default stream): `before`, s.synchronize(); a delay of DELAY_MS on `s` and the event `gate` behind
    it; the pending inputs are copied from their sources into the buffers; the outputs receive their initial contents (a zero-fill
    that ran early on stream 0 is overwritten here and shows as an error); `call`; the outputs are cloned.  All on `s`.
 4. On the host, before any wait: `gate` has not completed.  The host enqueued everything while the delay ran, so no call waited
    for the device -- the list of waiting calls in include/mcpc.h (Threading) is what `before` absorbs: the first run after a
    bind_target on an all-ReLU Bernoulli engine, the first accumulating run, the first evaluator call (its scratch).
 5. The canary: straight after the copies of step 3 are queued, one pending buffer is cloned on the DEFAULT stream.  After
    s.synchronize() that clone still holds the poison: work on stream 0 did overtake `s` in this run, so a mis-streamed launch would
    have read poison too.
 6. s.synchronize(), nothing wider; the clones are compared with `want` bit for bit.  Then torch.cuda.synchronize() and the engine's
    sync_check().
A facade case (PCTrainer) synchronises the host at its end, so step 4 does not apply to it; the canary alone shows the overtaking.

THE DELAY.  torch.cuda._sleep, calibrated once per process with two events around _sleep(10**6).  DELAY_MS is ten times the longest
host time any case needs between the start of the delay and the end of the clones (profiles/stream_cases.txt holds the per-case
figures), rounded up to 10 ms: host enqueue time jitters on a shared machine, and step 4 fails the case where it is still too short.
DELAY_MS = 10 ms.
"""
import functools
import time

import numpy as np

DELAY_MS = 10
EXCLUDED = ("mcpc_sync_check", "mcpc_debug_poison_lds", "mcpc_allreduce_grads")
HOST_MS = {}                              # case name -> host milliseconds of step 3 behind the delay, of the last run
F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64


# ---- poison and sentinels ---------------------------------------------------------------------------------------------------------------
def nan(shape, dtype=F32):
    return np.full(shape, np.nan, dtype=dtype)


def marked(shape, dtype=I64, value=0x0123456789):
    """An integer sentinel: what an output holds until the call under test overwrites it."""
    return np.full(shape, value, dtype=dtype)


def poison_of(case, name, a):
    """What the buffer of input ``name`` holds until the delayed copy lands."""
    if name in case.index:
        lo, hi, step = case.index[name]
        return (lo + (a.astype(np.int64) - lo + step) % (hi - lo)).astype(a.dtype)
    if a.dtype.kind != "f":
        raise TypeError(f"{case.name}: input {name!r} is not float data and not in the case's index table")
    return np.full_like(a, np.nan)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---- the scenario -----------------------------------------------------------------------------------------------------------------------
class Case:
    """One row of the table.  ``entries``: the functions of include/mcpc.h the case runs on the side stream.  ``index``: per input
    that is no float data, (lo, hi, step): its values lie in [lo, hi) and its poison is lo + (v - lo + step) % (hi - lo)."""
    name = None
    entries = ()
    index = {}
    pending = None                        # names of the pending inputs; None: every input
    scratch = ()                          # names of `outputs` whose contents are irrelevant (a workspace): not compared
    facade = False

    def inputs(self):                     # -> {name: ndarray}: the real inputs; no device needed
        raise NotImplementedError

    def outputs(self, src):               # -> {name: ndarray}: initial contents of outputs and accumulators
        return {}

    def before(self, dev, src):           # engines, binds, warm-up; on the current stream; -> state
        return None

    def call(self, st, buf, out):         # the call(s) under test; -> {name: tensor} compared besides `out`
        raise NotImplementedError

    def after(self, st):
        eng = getattr(st, "eng", None)
        if eng is not None:
            eng.sync_check()
            eng.close()

    def pending_names(self):
        return tuple(self.inputs()) if self.pending is None else tuple(self.pending)


class Report:
    def __init__(self):
        self.gate_pending = None          # step 4: the delay was still running when the host had enqueued everything
        self.canary_holds = None          # step 5
        self.mismatches = []              # step 6: names of outputs whose bits differ from `want`
        self.host_ms = None

    def check(self, facade=False):
        assert facade or self.gate_pending, \
            f"the delay ended before the host had enqueued the case ({self.host_ms:.1f} ms of host time): a call waited, or DELAY_MS is too short"
        assert self.canary_holds, "the default stream did not overtake the side stream: the run proved nothing"
        assert not self.mismatches, f"differ from the default-stream run: {self.mismatches}"


@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    import torch
    torch.cuda._sleep(10 ** 6)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10 ** 6)
    e1.record()
    torch.cuda.synchronize()
    return 10 ** 6 / e0.elapsed_time(e1)


_STREAMS = []                             # every candidate stays alive: torch hands its pooled streams out round-robin


@functools.lru_cache(maxsize=None)
def side_stream(dev):
    """A torch.cuda.Stream() that the default stream can overtake.  The runtime multiplexes its streams over a few hardware queues
    (four by default), and a stream that shares the default stream's queue runs in submission order with it: nothing on stream 0
    would get ahead of its delay, the canary would not hold and the run would prove nothing.  Candidates are probed with a short
    delay; the first behind whose delay the default stream still drains is kept for the process."""
    import torch
    default = torch.cuda.default_stream(dev)
    cycles = int(20 * _cycles_per_ms())
    for _ in range(16):
        s = torch.cuda.Stream(dev)
        _STREAMS.append(s)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            gate = torch.cuda.Event()
            gate.record(s)
        with torch.cuda.stream(default):
            torch.zeros(8, device=dev)
        default.synchronize()
        overtook = not gate.query()
        torch.cuda.synchronize()
        if overtook:
            return s
    raise AssertionError("no side stream that the default stream overtakes: torch's side streams block stream 0 on this machine")


def _sequence(case, dev, src, init, side, delay_ms):
    """Steps 2 to 6 (``side``), or the same sequence on the default stream without a delay (step 1).  -> (outputs on the host, Report)"""
    import torch
    names = case.pending_names()
    buf = {k: torch.from_numpy(poison_of(case, k, case.inputs()[k])).to(dev) for k in names}
    out = {k: torch.empty_like(v) for k, v in init.items()}
    cycles = int(delay_ms * _cycles_per_ms()) if side else 0
    torch.cuda.synchronize()
    default = torch.cuda.default_stream(dev)
    s = side_stream(dev) if side else default
    rep = Report()
    canary = None
    with torch.cuda.stream(s):
        st = case.before(dev, src)
        s.synchronize()
        t0 = time.perf_counter()
        if side:
            torch.cuda._sleep(cycles)
            gate = torch.cuda.Event()
            gate.record(s)
        for k in names:
            buf[k].copy_(src[k])
        if side:
            with torch.cuda.stream(default):
                canary = buf[names[0]].clone()
        for k in out:
            out[k].copy_(init[k])
        got = {k: v for k, v in out.items() if k not in case.scratch}
        got.update(case.call(st, {**src, **buf}, out) or {})
        clones = {k: v.clone() for k, v in got.items()}
        rep.host_ms = (time.perf_counter() - t0) * 1e3
    if side:
        rep.gate_pending = not gate.query()
    s.synchronize()
    with torch.cuda.stream(s):
        res = {k: v.cpu().numpy() for k, v in clones.items()}
    if side:
        rep.canary_holds = same_bits(canary.cpu().numpy(), poison_of(case, names[0], case.inputs()[names[0]]))
    torch.cuda.synchronize()
    case.after(st)
    return res, rep


def run_scenario(case, dev="cuda:0", delay_ms=None):
    """The whole scenario of one case -> Report (``Report.check`` asserts steps 4, 5 and 6)."""
    import torch
    dev = torch.device(dev)
    src = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.inputs().items()}
    init = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in case.outputs(case.inputs()).items()}
    want, _ = _sequence(case, dev, src, init, False, 0)
    got, rep = _sequence(case, dev, src, init, True, DELAY_MS if delay_ms is None else delay_ms)
    assert sorted(got) == sorted(want) and got, (sorted(got), sorted(want))
    rep.mismatches = [k for k in sorted(want) if not same_bits(got[k], want[k])]
    HOST_MS[case.name] = rep.host_ms
    return rep


class _State:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---- engine cases -----------------------------------------------------------------------------------------------------------------------
def _net_inputs(seed, n_in, sizes, n_out, batch, target):
    """Seeded weights W<j> / biases b<j>, pseudo-inputs, target y and a state x<l> of a net, fp32."""
    rs = np.random.RandomState(seed)
    dims = [n_in] + list(sizes) + ([n_out] if n_out else [])
    d = {}
    for j in range(len(dims) - 1):
        d[f"W{j}"] = (rs.uniform(-1, 1, (dims[j + 1], dims[j])) / np.sqrt(dims[j])).astype(F32)
        d[f"b{j}"] = (rs.uniform(-1, 1, dims[j + 1]) / np.sqrt(dims[j])).astype(F32)
    d["inputs"] = (0.5 * rs.randn(batch, n_in)).astype(F32)
    if target == "binary":
        d["y"] = (rs.rand(batch, n_out) < 0.3).astype(F32)
    elif target == "normal":
        d["y"] = rs.randn(batch, n_out).astype(F32)
    for l, n in enumerate(sizes):
        d[f"x{l}"] = (0.5 * rs.uniform(-1, 1, (batch, n))).astype(F32)
    return d


def _seq(d, stem, n):
    return [d[f"{stem}{i}"] for i in range(n)]


class _EngineCase(Case):
    """A 16-16-16 -> 16 net (tests/test_gpu_run_plan.py's).  ``before`` creates the engine, binds the real weights and target and makes
    one warm-up run of ``warm`` on data of its own (half the state, another seed): the documented host waits -- the target's flags,
    the spill ring -- happen there, and what it leaves in the engine differs from what the call under test must produce."""
    sizes, n_in, n_out = (16, 16), 16, 16
    act, target, batch, tuning = "relu", "binary", 64, None
    pending = ("x0", "x1", "inputs")
    seed = 5

    def inputs(self):
        return self._inputs(self.batch_now())

    @functools.lru_cache(maxsize=None)
    def _inputs(self, batch):
        return _net_inputs(self.seed, self.n_in, self.sizes, self.n_out, batch, self.target)

    def batch_now(self):
        return self.batch

    def tuning_now(self):
        return self.tuning

    def run_kwargs(self, L):
        raise NotImplementedError

    def engine(self, dev, src, weights=None):
        from montecarlopredictivecoding_amd import _lib as L
        from montecarlopredictivecoding_amd.engine import Engine
        n = len(self.sizes)
        act = {"relu": L.ACT_RELU, "tanh": L.ACT_TANH}[self.act]
        eng = Engine(list(self.sizes), [act] * n, self.n_in, self.n_out, self.batch_now(), device=dev, tuning=self.tuning_now())
        eng.bind_params(weights[0] if weights else _seq(src, "W", n + 1), weights[1] if weights else _seq(src, "b", n + 1))
        return eng, L

    def before(self, dev, src):
        eng, L = self.engine(dev, src)
        warm = [0.5 * x for x in _seq(src, "x", len(self.sizes))]
        eng.bind_inputs(src["inputs"])
        eng.bind_target(src["y"])
        eng.load_state(warm)
        kw = dict(self.run_kwargs(L))
        kw["seed"] = kw.get("seed", 0) + 1
        eng.run(**kw)
        return _State(eng=eng, L=L, keep=warm)

    def load(self, st, buf):
        st.eng.bind_inputs(buf["inputs"])
        st.eng.load_state(_seq(buf, "x", len(self.sizes)))


class RunPlanCase(_EngineCase):
    """mcpc_run on one executor branch of tests/test_gpu_run_plan.py: T = 40, window [7, 33), SGD with the Philox kick, energies ALL,
    records of x and of the outputs; then the state and the flat gradient bucket."""
    entries = ("mcpc_run", "mcpc_bind_inputs", "mcpc_load_state", "mcpc_store_state", "mcpc_read_param_grads_flat")
    T, REC = 40, 5

    def __init__(self, plan):
        self.plan, self.name = plan, f"run[{plan}]"

    def _plan_case(self):
        from tests import test_gpu_run_plan as rp
        return rp._case(self.plan)

    def batch_now(self):
        return self._plan_case()[0]

    def tuning_now(self):
        return self._plan_case()[1]

    def run_kwargs(self, L):
        return dict(T=self.T, loss_kind=L.LOSS_BERNOULLI, lr=0.03, noise_mode=L.NOISE_PHILOX, seed=3, step_base=11, acc_begin=7,
                    acc_end=33, energy_mode=L.ENERGY_ALL, rec_begin=0, rec_stride=9, rec_count=self.REC, rec_x=True, rec_out=True)

    def outputs(self, src):
        B = src["x0"].shape[0]
        o = {"energies": nan((self.T, 8), F64), "rec_out": nan((self.REC, B, self.n_out))}
        for l, n in enumerate(self.sizes):
            o[f"rec{l}"], o[f"xs{l}"] = nan((self.REC, B, n)), nan((B, n))
        return o

    def call(self, st, buf, out):
        self.load(st, buf)
        st.eng.run(energies_out=out["energies"], rec_x_bufs=_seq(out, "rec", 2), rec_out_buf=out["rec_out"], **self.run_kwargs(st.L))
        st.eng.store_state(_seq(out, "xs", 2))
        return {"flat": st.eng.read_param_grads_flat()}


class AdamCase(_EngineCase):
    """mcpc_run with ws=3, Adam on x and no noise, on a tanh net, then store_adam_state; the target is pending too."""
    name = "run[ws=3,adam,tanh]"
    entries = ("mcpc_run", "mcpc_bind_target", "mcpc_store_adam_state", "mcpc_store_state")
    act, target, tuning = "tanh", "normal", "ws=3"
    pending = ("x0", "x1", "inputs", "y")

    def run_kwargs(self, L):
        return dict(T=12, loss_kind=L.LOSS_GAUSSIAN, loss_var=0.7, xopt=L.XOPT_ADAM, lr=0.02, noise_mode=L.NOISE_NONE,
                    energy_mode=L.ENERGY_LAST)

    def outputs(self, src):
        o = {"energies": nan((1, 8), F64)}
        for l, n in enumerate(self.sizes):
            o[f"m{l}"], o[f"v{l}"], o[f"xs{l}"] = nan((self.batch, n)), nan((self.batch, n)), nan((self.batch, n))
        return o

    def call(self, st, buf, out):
        self.load(st, buf)
        st.eng.bind_target(buf["y"])
        st.eng.run(energies_out=out["energies"], **self.run_kwargs(st.L))
        st.eng.store_adam_state(_seq(out, "m", 2), _seq(out, "v", 2))
        st.eng.store_state(_seq(out, "xs", 2))


class XgradCase(_EngineCase):
    name = "run[update_x=False]"
    entries = ("mcpc_run",)

    def run_kwargs(self, L):
        return dict(T=1, loss_kind=L.LOSS_BERNOULLI, update_x=False)

    def call(self, st, buf, out):
        self.load(st, buf)
        res = st.eng.run(**self.run_kwargs(st.L))
        return {f"xgrad{l}": g for l, g in enumerate(res.xgrad)}


class ParamsChangedCase(_EngineCase):
    """The bound weight tensors are rewritten on the side stream behind the delay, then params_changed(), then a run: it must see the
    new weights (until then the tensors, and the engine's packed copy of them, hold NaN)."""
    name = "params_changed"
    entries = ("mcpc_params_changed", "mcpc_run")
    act, target = "tanh", "normal"
    pending = ("W0", "b0", "W1", "b1", "W2", "b2", "x0", "x1", "inputs")

    def run_kwargs(self, L):
        return dict(T=6, loss_kind=L.LOSS_GAUSSIAN, lr=0.05, noise_mode=L.NOISE_PHILOX, seed=9, step_base=4, energy_mode=L.ENERGY_ALL)

    def outputs(self, src):
        return {"energies": nan((6, 8), F64), "xs0": nan((self.batch, 16)), "xs1": nan((self.batch, 16))}

    def before(self, dev, src):
        import torch
        W = [torch.full_like(w, float("nan")) for w in _seq(src, "W", 3)]
        b = [torch.full_like(v, float("nan")) for v in _seq(src, "b", 3)]
        eng, L = self.engine(dev, src, (W, b))
        eng.bind_inputs(src["inputs"])
        eng.bind_target(src["y"])
        eng.load_state(_seq(src, "x", 2))
        eng.run(**self.run_kwargs(L))
        return _State(eng=eng, L=L, W=W, b=b)

    def call(self, st, buf, out):
        for j in range(3):                                   # the optimizer's step: the bound tensors change in place
            st.W[j].copy_(buf[f"W{j}"])
            st.b[j].copy_(buf[f"b{j}"])
        st.eng.params_changed()
        self.load(st, buf)
        st.eng.run(energies_out=out["energies"], **self.run_kwargs(st.L))
        st.eng.store_state(_seq(out, "xs", 2))


class GradsCase(_EngineCase):
    """store_state, read_param_grads with accumulate=True into a pending dW / db, and read_param_grads_flat with a scale."""
    name = "param_grads"
    entries = ("mcpc_run", "mcpc_store_state", "mcpc_read_param_grads", "mcpc_read_param_grads_flat")

    def run_kwargs(self, L):
        return dict(T=10, loss_kind=L.LOSS_BERNOULLI, lr=0.03, noise_mode=L.NOISE_PHILOX, seed=21, step_base=2, acc_begin=2, acc_end=10)

    def outputs(self, src):
        rs = np.random.RandomState(77)
        o = {"xs0": nan((self.batch, 16)), "xs1": nan((self.batch, 16))}
        for j in range(3):
            o[f"dW{j}"], o[f"db{j}"] = rs.randn(16, 16).astype(F32), rs.randn(16).astype(F32)
        return o

    def call(self, st, buf, out):
        self.load(st, buf)
        st.eng.run(**self.run_kwargs(st.L))
        st.eng.store_state(_seq(out, "xs", 2))
        for j in range(3):
            st.eng.read_param_grads(j, out[f"dW{j}"], out[f"db{j}"], scale=0.5, accumulate=True)
        return {"flat": st.eng.read_param_grads_flat(scale=0.25)}


class EvaluatorCase(Case):
    """chain_energies, prediction_errors(quantity="both") and sample_prior(latents=True) on net relu_bern_mask of
    tests/chain_energy_cases.py, max_rows = 128 so that two chunks run (210 rows, 150 samples).  The warm-up calls allocate the
    engine's scratch (include/mcpc.h: "asynchronous on `stream` but for those allocations")."""
    NET, MAX_ROWS, N_SAMPLES = "relu_bern_mask", 128, 150

    def __init__(self, which):
        self.which, self.name = which, which
        self.entries = ("mcpc_" + which,)
        self.pending = ("prior_inputs",) if which == "sample_prior" else ("inputs", "x0", "x1", "x2")

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests import chain_energy_cases as cc
        d = cc.data(self.NET)
        out = {f"W{j}": d["W"][j] for j in range(4)}
        out.update({f"b{j}": d["b"][j] for j in range(4)})
        out.update({f"x{l}": d["xs"][l] for l in range(3)})
        out.update(inputs=d["inputs"], y=d["target"])
        out["prior_inputs"] = np.random.RandomState(6).randn(self.N_SAMPLES, cc.NETS[self.NET]["n_in"]).astype(F32)
        return {k: np.array(v) for k, v in out.items()}

    def outputs(self, src):
        B = src["inputs"].shape[0]
        if self.which == "chain_energies":
            return {"table": nan((3, B, 8), F64)}
        if self.which == "sample_prior":
            return {"readout": nan((self.N_SAMPLES, src["y"].shape[1]))}
        return {}

    def kwargs(self, L):
        from tests import chain_energy_cases as cc
        c = cc.NETS[self.NET]
        return c, dict(loss_kind=c["loss"], loss_var=c["var"], mask_start=c["mask_start"], max_rows=self.MAX_ROWS)

    def evaluate(self, st, d, out):
        c, kw = self.kwargs(st.L)
        if self.which == "chain_energies":
            return {"table": st.eng.chain_energies(d["inputs"], _seq(d, "x", 3), out=None if out is None else out["table"], **kw)}
        if self.which == "prediction_errors":
            return st.eng.prediction_errors(d["inputs"], _seq(d, "x", 3), quantity="both", outputs="both", **kw)
        o, xs = st.eng.sample_prior(self.N_SAMPLES, seed=12, step=3, sample_base=40, inputs=d["prior_inputs"], loss="bernoulli",
                                    readout="mean", latents=True, out=None if out is None else out["readout"], max_rows=self.MAX_ROWS)
        return {f"latent{l}": x for l, x in enumerate(xs)}

    def before(self, dev, src):
        from montecarlopredictivecoding_amd import _lib as L
        from montecarlopredictivecoding_amd.engine import Engine
        from tests import chain_energy_cases as cc
        c = cc.NETS[self.NET]
        eng = Engine(list(c["sizes"]), [c["act"]] * 3, c["n_in"], c["n_out"], c["B"], device=dev)
        eng.bind_params(_seq(src, "W", 4), _seq(src, "b", 4))
        eng.bind_inputs(None)
        eng.bind_target(src["y"])
        st = _State(eng=eng, L=L)
        self.evaluate(st, src, None)
        return st

    def call(self, st, buf, out):
        res = self.evaluate(st, buf, out)
        return {k: v for k, v in res.items() if k not in out}


# ---- stateless cases --------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([1905, *key])


def _rec(key, R, B, w, scale=1.5):
    return (scale * _rng(key, R, B, w).standard_normal((R, B, w))).astype(F32)


class PhiloxCase(Case):
    """No input is pending: the output buffer, written with a sentinel behind the delay, is what a launch on stream 0 loses."""
    name, entries = "philox_normals", ("mcpc_philox_normals",)

    def inputs(self):
        return {"unused": np.zeros(4, F32)}

    def outputs(self, src):
        return {"z": nan((19, 37))}

    def call(self, st, buf, out):
        import ctypes as C
        from montecarlopredictivecoding_amd import _lib as L
        from montecarlopredictivecoding_amd.engine import _current_stream
        z = out["z"]
        L.check(L.load().mcpc_philox_normals(z.device.index or 0, 77, 5, 1, 1000, 19, 37, C.c_void_p(z.data_ptr()), 0,
                                             _current_stream(z.device)))


class BoxMullerCase(Case):
    name, entries = "box_muller", ("mcpc_box_muller",)
    index = {"a": (-2 ** 31, 2 ** 31, 0x12345600), "b": (-2 ** 31, 2 ** 31, 0x0FEDCB00)}

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        bits = _rng(1).integers(-2 ** 31, 2 ** 31, (2, 1001), dtype=np.int64).astype(I32)
        return {"a": bits[0], "b": bits[1]}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import box_muller
        z0, z1 = box_muller(buf["a"], buf["b"])
        return {"z0": z0, "z1": z1}


class MomentsCase(Case):
    """sum and sumsq with the sigmoid transform at row_elems = 15 (odd: the scalar form), added to a prior state."""
    name, entries = "moments_accumulate", ("mcpc_moments_accumulate",)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        return {"rec": _rec(2, 7, 3, 5)}

    def outputs(self, src):
        r = _rng(2, 1)
        return {"sum": r.standard_normal(15), "sumsq": r.standard_normal(15) ** 2}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import moments_accumulate
        moments_accumulate(buf["rec"], 1, 2, 3, out["sum"], out["sumsq"], transform="sigmoid", accumulate=True)


class CovCase(Case):
    """accumulate=False, so the zero-fill runs; two blocks of widths 17 and 33."""
    entries = ("mcpc_cov_accumulate",)

    def __init__(self, pool):
        self.pool, self.name = pool, "cov_accumulate[%s]" % ("pooled" if pool else "per chain")

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        return {"r0": _rec(3, 5, 3, 17), "r1": _rec(4, 5, 3, 33)}

    def outputs(self, src):
        return {"outer": nan((50, 50) if self.pool else (3, 50, 50), F64)}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import cov_accumulate
        cov_accumulate([buf["r0"], buf["r1"]], 0, 1, 5, out["outer"], transforms=["identity", "sigmoid"], pool=self.pool, accumulate=False)


class HistCase(Case):
    entries = ("mcpc_hist_accumulate",)
    EDGES = np.linspace(-2.0, 2.0, 8).astype(F32)

    def __init__(self, pool):
        self.pool, self.name = pool, "hist_accumulate[%s]" % ("pooled" if pool else "per chain")

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        return {"rec": _rec(5, 6, 3, 5)}

    def outputs(self, src):
        return {"counts": marked((5, 10) if self.pool else (3, 5, 10))}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import hist_accumulate
        hist_accumulate(buf["rec"], 0, 1, 6, self.EDGES, out["counts"], pool=self.pool, accumulate=False)


class Hist2dCase(Case):
    name, entries = "hist2d_accumulate", ("mcpc_hist2d_accumulate",)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        return {"rx": _rec(6, 6, 3, 5), "ry": _rec(7, 6, 3, 4)}

    def outputs(self, src):
        return {"counts": marked((3, 3, 10, 8))}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import hist2d_accumulate
        hist2d_accumulate(buf["rx"], buf["ry"], 0, 1, 6, [(0, 1), (4, 3), (2, 2)], HistCase.EDGES, np.linspace(-1.5, 1.5, 6).astype(F32),
                          out["counts"], accumulate=False)


class AcovCase(Case):
    """A fresh stream (n_seen = 0: lagged and sum are overwritten) and a continued one (every piece of the state is pending)."""
    entries = ("mcpc_acov_accumulate",)
    K, B, W = 3, 3, 5

    def __init__(self, n_seen):
        self.n_seen, self.name = n_seen, "acov_accumulate[%s]" % ("continued" if n_seen else "fresh")

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests.acov_cases import ar1
        series = np.stack([ar1(0.6, 8, 0.3, 40 + e) for e in range(self.B * self.W)], axis=1)
        return {"rec": series.reshape(8, self.B, self.W)}

    def outputs(self, src):
        K, B, W = self.K, self.B, self.W
        if not self.n_seen:
            return {"lagged": nan((B, W, K + 1), F64), "sum": nan((B, W), F64), "window": nan((K, B, W)), "head": nan((K, B, W))}
        r = _rng(8)
        return {"lagged": r.standard_normal((B, W, K + 1)), "sum": r.standard_normal((B, W)),
                "window": r.standard_normal((K, B, W)).astype(F32), "head": r.standard_normal((K, B, W)).astype(F32)}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import acov_accumulate
        acov_accumulate(buf["rec"], 1, 1, 5, self.K, self.n_seen, out["lagged"], out["sum"], out["window"], out["head"])


class RollCase(Case):
    """out_pool through a caller's workspace, the stream continued across two calls (4 + 5 samples, window 3)."""
    name, entries = "roll_accumulate", ("mcpc_roll_accumulate",)
    scratch = ("workspace",)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests.roll_cases import noise
        return {"rec": noise(9, 15, 11).reshape(9, 3, 5)}

    def outputs(self, src):
        return {"s1": nan((3, 5), F64), "s2": nan((3, 5), F64), "hist": nan((3, 3, 5)), "elem": nan((7, 3, 5), F64),
                "pool_a": nan((2, 4), F64), "pool_b": nan((5, 4), F64), "workspace": np.zeros(1 << 16, np.uint8)}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import roll_accumulate
        a = roll_accumulate(buf["rec"], 0, 1, 4, 3, 1, 0, out["s1"], out["s2"], out["hist"], out["elem"][:2], out["pool_a"], out["workspace"])
        b = roll_accumulate(buf["rec"], 4, 1, 5, 3, 1, 4, out["s1"], out["s2"], out["hist"], out["elem"][2:], out["pool_b"], out["workspace"])
        assert (a, b) == (2, 5)


class ProbeCase(Case):
    def __init__(self, records):
        self.records = records
        self.name = "probe_records" if records else "probe_accumulate"
        self.entries = ("mcpc_" + self.name,)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        r = _rng(9)
        return {"rec": _rec(9, 6, 3, 5), "W": r.standard_normal((4, 5)).astype(F32), "bias": r.standard_normal(4).astype(F32)}

    def outputs(self, src):
        if self.records:
            return {"p": nan((3, 3, 4))}
        return {"psum": nan((3, 4), F64), "psumsq": nan((3, 4), F64), "votes": marked((3, 5)), "entsum": nan((3,), F64)}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd import engine as E
        if self.records:
            E.probe_records(buf["rec"], 1, 2, 3, buf["W"], buf["bias"], "softmax", out=out["p"])
        else:
            E.probe_accumulate(buf["rec"], 0, 1, 6, buf["W"], buf["bias"], "softmax", out["psum"], out["psumsq"], out["votes"],
                               out["entsum"], accumulate=False)


class KnnCase(Case):
    """Two reference chunks, the second with accumulate=True."""
    name, entries = "knn_accumulate", ("mcpc_knn_accumulate",)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        r = _rng(10)
        return {"q": r.standard_normal((7, 3)).astype(F32), "ref_a": r.standard_normal((11, 3)).astype(F32),
                "ref_b": r.standard_normal((9, 3)).astype(F32)}

    def outputs(self, src):
        return {"best": nan((7, 2))}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import knn_accumulate
        knn_accumulate(buf["q"], buf["ref_a"], 2, out["best"], accumulate=False)
        knn_accumulate(buf["q"], buf["ref_b"], 2, out["best"], accumulate=True)


class LoglikCase(Case):
    name, entries = "loglik_accumulate", ("mcpc_loglik_accumulate",)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests.loglik_cases import make_case
        y, o, _ = make_case(5, 33, 7, "bernoulli")
        return {"y": y, "o": o}

    def outputs(self, src):
        return {"state": nan((5, 4), F64)}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import loglik_accumulate
        loglik_accumulate(buf["y"], buf["o"], "bernoulli", None, 20.0, out["state"], accumulate=False)


class AisIncrementCase(Case):
    name, entries = "ais_increment", ("mcpc_ais_increment",)
    CASE = "relu_bern_masked"

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests.ais_cases import increment_inputs
        x, W, bias, y, _ = increment_inputs(self.CASE)
        return {"x": np.array(x), "W": np.array(W), "bias": np.array(bias), "y": np.array(y)}

    def outputs(self, src):
        from tests.ais_cases import increment_inputs
        return {"logw": np.array(increment_inputs(self.CASE)[4])}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import ais_increment
        from tests.ais_cases import INCREMENT_CASES, RUNGS
        c = INCREMENT_CASES[self.CASE]
        ais_increment(buf["x"], buf["W"], buf["bias"], buf["y"], c["act"], c["loss"], c["var"], c["mask_start"],
                      *RUNGS[c["loss"]]["middle"], out["logw"], accumulate=True)


def _layers(stem, arrays):
    return {f"{stem}{l}": np.array(a) for l, a in enumerate(arrays)}


class MalaCase(Case):
    """mala_propose, and mala_accept with x_next, on tests/mala_cases.py's three-layer case; the state the decision overwrites in
    place is pending as well."""
    NET = "three_layers"

    def __init__(self, accept):
        self.accept = accept
        self.name = "mala_accept" if accept else "mala_propose"
        self.entries = ("mcpc_" + self.name,)
        self.pending = ("xp0", "xp1", "xp2", "gp0", "gp1", "gp2", "Ep") if accept else None

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests.mala_cases import kernel_inputs
        xs, gs, E, xps, gps, Ep = kernel_inputs(self.NET)
        d = {**_layers("x", xs), **_layers("g", gs)}
        if self.accept:
            d.update({**_layers("xp", xps), **_layers("gp", gps), "E": np.array(E), "Ep": np.array(Ep)})
        return d

    def outputs(self, src):
        if not self.accept:
            return {f"out{l}": nan(src[f"x{l}"].shape) for l in range(3)}
        o = {k: src[k] for k in ("x0", "x1", "x2", "g0", "g1", "g2", "E")}           # overwritten in place: the prior state
        o.update({f"next{l}": nan(src[f"x{l}"].shape) for l in range(3)})
        o.update(diag=nan((src["E"].shape[0], 3), F64), n_accepted=np.arange(src["E"].shape[0], dtype=I32))
        return o

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd import engine as E
        from tests.mala_cases import KERNEL_RUN
        if not self.accept:
            E.mala_propose(_seq(buf, "x", 3), _seq(buf, "g", 3), out=_seq(out, "out", 3), **KERNEL_RUN)
        else:
            E.mala_accept(_seq(out, "x", 3), _seq(out, "g", 3), out["E"], _seq(buf, "xp", 3), _seq(buf, "gp", 3), buf["Ep"],
                          diag=out["diag"], n_accepted=out["n_accepted"], x_next=_seq(out, "next", 3), **KERNEL_RUN)


class HmcCase(Case):
    """hmc_begin, hmc_leap and hmc_accept as one trajectory of two leapfrog steps (the gradients along it are given)."""
    name, entries = "hmc_trajectory", ("mcpc_hmc_begin", "mcpc_hmc_leap", "mcpc_hmc_accept")
    NET = "three_layers"
    pending = ("gt0", "gt1", "gt2", "gu0", "gu1", "gu2", "Et")

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests.hmc_cases import kernel_inputs
        xs, gs, E, xts, gts, Et, qs, K0 = kernel_inputs(self.NET)
        r = _rng(12)
        gus = [r.standard_normal(g.shape).astype(F32) for g in gts]
        return {**_layers("x", xs), **_layers("g", gs), **_layers("gt", gts), **_layers("gu", gus), "E": np.array(E), "Et": np.array(Et)}

    def outputs(self, src):
        rows = src["E"].shape[0]
        o = {k: src[k] for k in ("x0", "x1", "x2", "g0", "g1", "g2", "E")}
        for l in range(3):
            o[f"q{l}"], o[f"xt{l}"] = nan(src[f"x{l}"].shape), nan(src[f"x{l}"].shape)
        o.update(K0=nan((rows,), F64), diag=nan((rows, 3), F64), n_accepted=np.arange(rows, dtype=I32))
        return o

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd import engine as E
        from tests.hmc_cases import KERNEL_RUN as R
        xs, gs, qs, xts = _seq(out, "x", 3), _seq(out, "g", 3), _seq(out, "q", 3), _seq(out, "xt", 3)
        E.hmc_begin(xs, gs, R["lr"], R["seed"], R["step"], R["chain_base"], q_out=qs, x_out=xts, K0=out["K0"])
        E.hmc_leap(xts, qs, _seq(buf, "gt", 3), R["lr"])
        E.hmc_accept(xs, gs, out["E"], xts, _seq(buf, "gu", 3), buf["Et"], qs, out["K0"], R["lr"], R["seed"], R["step"], R["chain_base"],
                     diag=out["diag"], n_accepted=out["n_accepted"])


class SmcAncestorsCase(Case):
    """Five data of 16 replicas at threshold 0.5: tests/smc_cases.py's spreads put some below the ESS threshold and some above.  The
    log-weights, rewritten in place, are the pending input (NaN poison: a datum without a finite weight is left untouched)."""
    name, entries = "smc_ancestors", ("mcpc_smc_ancestors",)
    R, N = 16, 5

    def inputs(self):
        return {"unused": np.zeros(4, F32)}

    def outputs(self, src):
        from tests.smc_cases import kernel_logw
        return {"logw": np.array(kernel_logw(self.R, self.N)), "ancestors": marked((self.R * self.N,), I32, 0x1234567),
                "diag": nan((self.N, 4), F64)}

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import smc_ancestors
        from tests.smc_cases import KERNEL_RUN
        smc_ancestors(out["logw"], self.R, 0.5, ancestors=out["ancestors"], diag=out["diag"], **KERNEL_RUN)


class SmcGatherCase(Case):
    """The ancestors are an index: their poison is another row of the state, never one outside it."""
    name, entries = "smc_gather", ("mcpc_smc_gather",)
    ROWS, WIDTHS = 19, (5, 33, 17)
    index = {"ancestors": (0, ROWS, 1)}

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        r = _rng(13)
        d = {f"x{l}": r.standard_normal((self.ROWS, n)).astype(F32) for l, n in enumerate(self.WIDTHS)}
        d["ancestors"] = r.integers(0, self.ROWS, self.ROWS).astype(I32)
        return d

    def outputs(self, src):
        o = {f"out{l}": nan((self.ROWS, n)) for l, n in enumerate(self.WIDTHS)}
        o["n_bad"] = np.array([5], dtype=I32)
        return o

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd.engine import smc_gather
        smc_gather(_seq(buf, "x", 3), buf["ancestors"], out=_seq(out, "out", 3), n_bad=out["n_bad"])


# ---- facade cases ------------------------------------------------------------------------------------------------------------------------
def tensors_of(obj, prefix, found=None, seen=None, depth=0):
    """Every tensor and number reachable from a result (dicts, sequences, attributes of result objects), by a dotted name."""
    import torch
    found = {} if found is None else found
    seen = set() if seen is None else seen
    if isinstance(obj, torch.Tensor):
        found[prefix] = obj.detach()
    elif isinstance(obj, (bool, int, float)):
        found[prefix] = torch.tensor(float(obj), dtype=torch.float64)
    elif obj is None or isinstance(obj, (str, bytes)) or id(obj) in seen or depth > 6:
        pass
    elif isinstance(obj, dict):
        seen.add(id(obj))
        for k, v in obj.items():
            tensors_of(v, f"{prefix}.{k}", found, seen, depth + 1)
    elif isinstance(obj, (list, tuple)):
        seen.add(id(obj))
        for i, v in enumerate(obj):
            tensors_of(v, f"{prefix}.{i}", found, seen, depth + 1)
    elif hasattr(obj, "__dict__") and not callable(obj) and not isinstance(obj, torch.nn.Module):
        seen.add(id(obj))
        for k, v in vars(obj).items():
            if not k.startswith("_"):
                tensors_of(v, f"{prefix}.{k}", found, seen, depth + 1)
    return found


class TrainOnBatchCase(Case):
    """PCTrainer.train_on_batch, a fused learning call on tests/test_gpu_roll_facade.py's net (5-12-9 -> 14, 37 chains, T = 60,
    parameter sums over [40, 60)) with moments, a pooled covariance, a histogram and the rolling variance asked for, the moments
    on the call's own stream or on the driver's side stream, x recorded on every step (the pinned-host drain) and a chunk budget of
    7 steps (at least three slices).  `inputs` and `_target` are pending.  The returned energies and records, every mcpc_last_*
    and every parameter behind the call's optimizer step are compared: the step has consumed param.grad (it is None afterwards, as in
    the reference), and the stepped parameter is a function of it; a gradient that is still there is compared too."""
    facade = True
    pending = ("inputs", "y")

    def __init__(self, side):
        self.side, self.name = side, f"train_on_batch[moments_side_stream={side}]"

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        r = _rng(14)
        return {"inputs": (0.5 * r.standard_normal((37, 5))).astype(F32), "y": (r.random((37, 14)) < 0.3).astype(F32)}

    def before(self, dev, src):
        from tests import test_gpu_roll_facade as rf
        um, model, _, _ = rf._net(str(dev))
        tr = rf._trainer(model, "last")
        tr.mcpc_moments = dict(rf.OTHERS["mcpc_moments"])
        tr.mcpc_covariance = dict(rf.OTHERS["mcpc_covariance"], pool="chains")
        tr.mcpc_histogram = dict(rf.OTHERS["mcpc_histogram"])
        tr.mcpc_rolling = dict(rf.SPEC)
        tr.mcpc_moments_side_stream = self.side
        tr.mcpc_moments_chunk_bytes = 7 * 4 * rf.B * (rf.SIZES[0] + rf.SIZES[2] + rf.N_OUT)
        return _State(rf=rf, um=um, model=model, tr=tr)

    def call(self, st, buf, out):
        import warnings
        import montecarlopredictivecoding_amd.predictive_coding.pc_trainer as pt
        tr, um = st.tr, st.um
        base = pt._PHILOX_STEPS[0]
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = tr.train_on_batch(inputs=buf["inputs"], callback_after_t=um.random_step, callback_after_t_kwargs={"_pc_trainer": tr},
                                        is_log_progress=False, is_return_results_every_t=True, is_return_xs=True, is_return_outputs=True,
                                        is_sample_x_at_batch_start=True, loss_fn=um.bernoulli_fn,
                                        loss_fn_kwargs={"_target": buf["y"], "_var": None})
        finally:
            pt._PHILOX_STEPS[0] = base                       # the next run replays the same noise
        assert tr.last_call_mode == "fused" and tr.last_record_slices >= 3, (tr.last_call_mode, tr.last_record_slices)
        got = tensors_of(res, "results")
        for attr in sorted(vars(tr)):
            if attr.startswith("mcpc_last_"):
                tensors_of(getattr(tr, attr), attr, got)
        for i, p in enumerate(st.model.parameters()):
            got[f"param{i}"] = p.detach()                     # after optimizer_p's step, which consumed param.grad (None behind it)
            if p.grad is not None:
                got[f"param{i}.grad"] = p.grad
        for attr in ("mcpc_last_moments", "mcpc_last_covariance", "mcpc_last_histogram", "mcpc_last_rolling"):
            assert sum(k.startswith(attr + ".") for k in got) >= 2, (attr, sorted(got))
        return got


class AisFacadeCase(Case):
    """PCTrainer.mcpc_ais (ais.run, for its optional returns) on tests/ais_cases.py's bern_relu net with pending `data`; the state,
    the raw log-weights, the accepted counts and the ancestors are compared."""
    facade = True
    FORMS = {"plain": {}, "mala,leapfrog=2": dict(adjust="mala", leapfrog=2), "systematic": dict(resample="systematic", ess_threshold=1.0)}

    def __init__(self, form):
        self.form, self.name = form, f"mcpc_ais[{form}]"

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        from tests import ais_cases as A
        return {"data": np.array(A.estimator_params("bern_relu")[2])}

    def before(self, dev, src):
        from tests.test_gpu_ais import case_trainer
        _, trainer, loss_fn, kw, _ = case_trainer("bern_relu")
        return _State(trainer=trainer, loss_fn=loss_fn, kw=kw)

    def call(self, st, buf, out):
        from montecarlopredictivecoding_amd import ais
        from tests import ais_cases as A
        ll, logw, acc, anc = ais.run(st.trainer, buf["data"], st.loss_fn, st.kw, return_logw=True, return_accepted=True,
                                     return_ancestors=True, **dict(A.ESTIMATOR_RUN, **self.FORMS[self.form]))
        got = {"state": ll.state, "logw": logw}
        assert (acc is not None) == ("mala" in self.form) and (anc is not None) == (self.form == "systematic")
        if acc is not None:
            got["accepted"] = acc
        if anc is not None:
            got["ancestors"] = anc
        return got


class OnTheDefaultStream(Case):
    """The scenario's own teeth: a plain torch op issued on the DEFAULT stream from inside the scenario.  No library code runs; the
    scenario must report the output as a mismatch (tests/test_gpu_streams.py)."""
    name, entries = "torch op on the default stream", ()

    def inputs(self):
        return {"x": np.arange(1, 1025, dtype=F32)}

    def outputs(self, src):
        return {"y": nan((1024,))}

    def call(self, st, buf, out):
        import torch
        with torch.cuda.stream(torch.cuda.default_stream(buf["x"].device)):
            torch.mul(buf["x"], 2.0, out=out["y"])


CASES = [RunPlanCase(p) for p in ("small", "small,no_overlap=1", "small,ws=0", "small,ws=4", "more")]
CASES += [AdamCase(), XgradCase(), ParamsChangedCase(), GradsCase()]
CASES += [EvaluatorCase(w) for w in ("chain_energies", "prediction_errors", "sample_prior")]
CASES += [PhiloxCase(), BoxMullerCase(), MomentsCase(), CovCase(True), CovCase(False), HistCase(True), HistCase(False), Hist2dCase(),
          AcovCase(0), AcovCase(4), RollCase(), ProbeCase(False), ProbeCase(True), KnnCase(), LoglikCase(), AisIncrementCase(),
          MalaCase(False), MalaCase(True), HmcCase(), SmcAncestorsCase(), SmcGatherCase()]
CASES += [TrainOnBatchCase(False), TrainOnBatchCase(True)] + [AisFacadeCase(f) for f in AisFacadeCase.FORMS]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

"""What mcpc_create would decide for a network and what mcpc_run would issue for a run on it, without a device: include/mcpc.h:
mcpc_debug_plan and mcpc_debug_run_plan through the loaded library."""
import ctypes as C
import json


def _net_desc(sizes, n_out, batch, tuning, n_in, spill_budget_bytes):
    from montecarlopredictivecoding_amd import _lib
    d = _lib.NetDesc()
    d.abi_version, d.n_latent, d.n_in, d.n_out, d.batch, d.device = _lib.ABI_VERSION, len(sizes), n_in, n_out, batch, 0
    for l, n in enumerate(sizes):
        d.sizes[l], d.acts[l], d.ecoef[l] = n, _lib.ACT_RELU, 1.0
    d.spill_budget_bytes = spill_budget_bytes
    d.tuning = tuning.encode() if tuning else None
    return d


def plan(sizes, n_out, batch, tuning=None, n_cu=256, total_mem=288 << 30, n_in=10, spill_budget_bytes=0):
    """The plan as a dict (see include/mcpc.h for its keys); raises _lib.MCPCError with mcpc_create's code and message."""
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    d = _net_desc(sizes, n_out, batch, tuning, n_in, spill_budget_bytes)
    need = C.c_int64()
    _lib.check(lib.mcpc_debug_plan(C.byref(d), n_cu, total_mem, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _lib.check(lib.mcpc_debug_plan(C.byref(d), n_cu, total_mem, buf, need.value, C.byref(need)))
    return json.loads(buf.value.decode())


def run_plan(sizes, n_out, batch, run, tuning=None, n_cu=256, total_mem=288 << 30, n_in=10, spill_budget_bytes=0):
    """The schedule of a run as a dict (include/mcpc.h: mcpc_debug_run_plan).  `run`: the fields of mcpc_run_desc that shape it, by name
    (T, t_begin, n_steps, acc_begin, acc_end, update_x, xopt_kind, noise_mode, loss_kind); every other field stays zero."""
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    d = _net_desc(sizes, n_out, batch, tuning, n_in, spill_budget_bytes)
    r = _lib.RunDesc()
    for key, val in run.items():
        setattr(r, key, val)
    need = C.c_int64()
    _lib.check(lib.mcpc_debug_run_plan(C.byref(d), n_cu, total_mem, C.byref(r), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _lib.check(lib.mcpc_debug_run_plan(C.byref(d), n_cu, total_mem, C.byref(r), buf, need.value, C.byref(need)))
    return json.loads(buf.value.decode())


def entries(step_plan):
    """The table of a step plan as a list of dicts, one per entry (row-major: the unified table's rows follow each other)."""
    return [dict(zip(step_plan["fields"], row)) for row in step_plan["table"]]

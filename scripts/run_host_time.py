#!/usr/bin/env python3
"""Host time of a learning call with many short Hebbian segments: how long Engine.run (mcpc_run inside it) takes to RETURN, without
waiting for the device.  cfg-M's net at 256 chains, T = 600 steps all accumulating, tuning slot_cap=6: ring parts of 2 slots, 300
segments and 300 flushes per call, so planning and issuing the flushes is most of what the host does.  One process = two warm-up
calls, then RUNS timed calls (the device is drained before each); prints their median in ms on one line.  For an A/B, run processes
of the two libraries alternately (MCPC_LIB=scripts/bin/libmcpc_<commit>.so for an earlier commit: scripts/build_old_lib.sh).

    python3 scripts/run_host_time.py [RUNS]
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_problem  # noqa: E402
from montecarlopredictivecoding_amd import _lib as L  # noqa: E402
from montecarlopredictivecoding_amd.engine import Engine  # noqa: E402

DEV = "cuda:0"
B, T = 256, 600
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
W, b, y, xs = make_problem(B, 30, DEV)
xs = [x * 0.1 for x in xs]
eng = Engine([30, 256, 256], [L.ACT_RELU] * 3, 30, 784, B, device=DEV, tuning="slot_cap=6")
eng.bind_params(W, b); eng.bind_inputs(None); eng.bind_target(y)
times = []
for i in range(2 + runs):
    eng.load_state(xs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(T, loss_kind=L.LOSS_BERNOULLI, lr=0.03, noise_mode=L.NOISE_PHILOX, seed=3, step_base=0, acc_begin=0, acc_end=T,
            energy_mode=L.ENERGY_LAST)
    dt = time.perf_counter() - t0
    eng.sync_check()
    if i >= 2:
        times.append(dt * 1e3)
assert eng.query()["spill_slots"] == 6
eng.close()
print("host time of the call: median %.3f ms  (min %.3f, max %.3f, %d calls; %s)" % (
    statistics.median(times), min(times), max(times), runs, os.path.basename(L.build_info()["path"])), flush=True)

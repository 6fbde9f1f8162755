"""What mcpc_create built is what the host planner says it builds (include/mcpc.h: mcpc_debug_plan, for the device's own CU count): ties
tests/test_plan_host.py and tests/test_round_plan.py, which need no GPU, to the engine.  Creates engines only; no run."""
import pytest
import torch

from tests.plan_util import plan

pytestmark = pytest.mark.gpu
BUDGET = 1 << 30        # an explicit spill budget: the device's memory plays no part


def _nets(n_cu):
    return [dict(sizes=[6, 16, 16], n_out=24, batch=40), dict(sizes=[20, 128, 128], n_out=784, batch=256),
            dict(sizes=[30, 200, 208], n_out=100, batch=33, tuning="ws=0"), dict(sizes=[30, 640, 640], n_out=784, batch=70, tuning="wide=1"),
            dict(sizes=[6, 16, 16], n_out=24, batch=16 * (n_cu + 1))]


def test_the_engine_is_what_the_planner_planned():
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    forms = []
    for net in _nets(n_cu):
        p = plan(n_cu=n_cu, total_mem=0, n_in=10, spill_budget_bytes=BUDGET, **net)
        eng = Engine(net["sizes"], [L.ACT_RELU] * len(net["sizes"]), 10, net["n_out"], net["batch"], device=torch.device("cuda", 0),
                     spill_budget_bytes=BUDGET, tuning=net.get("tuning", ""))
        try:
            q = eng.query()
        finally:
            eng.close()
        want = dict(lds_bytes=p["main"]["lds_bytes"], chains_per_wg=p["chains_per_wg"], n_workgroups=p["workgroups"], spill_slots=p["slots"],
                    step_kernel=p["kernel"])
        assert q == want, (net, q, want)
        forms.append((p["form"], p["unified"]["prefer"], p["rounds"]["on"]))
    # the five nets reach the five forms an engine can take
    assert forms == [("in-place", 1, 0), ("in-place", 1, 0), ("barrier", 0, 0), ("layer-wise", 0, 0), ("in-place", 1, 1)], forms

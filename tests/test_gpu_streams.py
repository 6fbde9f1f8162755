"""Every entry point on a side stream whose inputs are still pending (tests/stream_cases.py holds the scenario and the table).

A case passes when the host enqueued it while the side stream's delay was still running (no call waited for the device), the canary
shows that the default stream overtook the side stream in this very run, and every output is bitwise what the same sequence gives
on the default stream.  A launch, zero-fill or finish kernel on another stream than the one it was given reads poison or is
overwritten by the sentinel, and the case fails on the comparison."""
import pytest

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_on_a_side_stream_with_pending_inputs(name):
    case = sc.BY_NAME[name]
    rep = sc.run_scenario(case)
    print(f"{name}: host {rep.host_ms:.2f} ms behind the start of a delay of {sc.DELAY_MS} ms; gate pending {rep.gate_pending}, "
          f"canary holds {rep.canary_holds}, mismatches {rep.mismatches}")
    rep.check(facade=case.facade)


def test_the_scenario_catches_work_on_the_default_stream():
    """No library code: a torch op issued on the default stream from inside the scenario runs ahead of the delayed copies and is
    then overwritten by the sentinel.  The scenario must say so, and for that reason alone."""
    rep = sc.run_scenario(sc.OnTheDefaultStream())
    assert rep.gate_pending and rep.canary_holds
    assert rep.mismatches == ["y"]
    with pytest.raises(AssertionError, match="differ from the default-stream run"):
        rep.check()

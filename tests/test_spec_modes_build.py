"""What the specialised instantiations of the in-place step kernel are for, asserted from `make asm` (as tests/test_build_info.py
does for the generic kernel): fixing a launch's decisions at compile time must take SGPR pressure away -- strictly fewer spilled
SGPRs than the generic kernel, no spilled VGPR, no larger frame.  The numbers themselves: profiles/spec_modes.txt."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")


def test_specialised_step_kernels_spill_less_than_the_generic_one(tmp_path):
    asm = str(tmp_path / "mcpc_gfx950.s")
    run = subprocess.run(["make", "-C", CSRC, "asm", f"ASM_OUT={asm}"], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    usage, name = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    generic = {k: v for k, v in usage.items() if "mcpc_steps_ws2_kernelILi1E" in k}
    spec = {k: v for k, v in usage.items() if "mcpc_steps_ws2_spec_kernel" in k}
    assert len(generic) == 2, sorted(usage)
    # the hot set (without spill and with it) and the MAP warm-up's mode, each as plain launch and round schedule
    assert len(spec) == 6, sorted(spec)
    for k, u in spec.items():
        mix = k.endswith("Lb1EEEvNS_7KParamsE")
        (gk, g), = [(n, v) for n, v in generic.items() if n.endswith("Lb1EEEvNS_7KParamsE") == mix]
        print(f"{k}: {u}\n  against {gk}: {g}")
        assert u["VGPRs Spill"] == 0, (k, u)
        assert u["ScratchSize"] <= g["ScratchSize"], (k, u, g)
        assert u["SGPRs Spill"] < g["SGPRs Spill"], (k, u, g)

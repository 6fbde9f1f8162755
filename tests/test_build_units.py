"""libmcpc.so is built from separate translation units, one per concern (csrc/Makefile, csrc/mcpc_api.hip):

* a kernel exists once in the library -- no kernel name appears in two units (`make asm`: the units' device code side by side);
* every entry point of include/mcpc.h that the binding resolves is exported by the linked library, whichever unit defines it;
* the records unit (the stateless reducers) sees nothing of the engine, the planner or the step kernels;
* the run unit (mcpc_run and its executor) sees no kernel header and reaches the step kernels through launchers only;
* an edit recompiles the units that include the edited file, the build-info unit (so that the reported source hash is the tree's) and
  nothing else -- planned with `make -n -W <file>`, which modifies nothing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "montecarlopredictivecoding_amd")
CSRC = os.path.join(PKG, "csrc")
OBJDIR = os.path.join(PKG, "build", "product")
STEP_UNITS = ("mcpc_steps_ws2", "mcpc_steps_ws2_spec", "mcpc_steps_u", "mcpc_steps_lw")
UNITS = ("mcpc_api", "mcpc_run") + STEP_UNITS + ("mcpc_eval", "mcpc_flush", "mcpc_records", "mcpc_build_info")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """The product library, up to date (a no-op after build()), and one `make asm`: both shared by the whole file."""
    run = subprocess.run(["make", "-C", CSRC], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    asm = str(tmp_path_factory.mktemp("asm") / "mcpc_gfx950.s")
    run = subprocess.run(["make", "-C", CSRC, "asm", f"ASM_OUT={asm}"], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    return {"asm": open(asm).read(), "remarks": run.stderr}


def test_no_kernel_is_compiled_into_two_units(built):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", built["asm"], flags=re.M)
    assert len(names) > 100, "the scan found too few kernels: the pattern is broken"
    twice = sorted({n for n in names if names.count(n) > 1})
    assert not twice, f"kernels defined in more than one translation unit: {twice}"
    # and the remarks of `make asm` name every one of them once: the units' stderr is not mixed
    remarked = re.findall(r"remark: Function Name: (\S+)", built["remarks"])
    assert sorted(remarked) == sorted(names)


def test_every_bound_symbol_is_exported(built):
    from montecarlopredictivecoding_amd import _lib
    run = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libmcpc.so")], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in run.stdout.splitlines() if line.split()}
    missing = sorted(set(_lib.SYMBOLS) - exported)
    assert not missing, f"not exported by libmcpc.so: {missing}"


def test_records_unit_stands_apart(built):
    dep = open(os.path.join(OBJDIR, "mcpc_records.d")).read()
    seen = set(re.findall(r"(mcpc_\w+\.(?:h|inc))", dep))
    assert "mcpc_hist.h" in seen and "mcpc_host.h" in seen, "the depfile does not name the unit's own headers: the pattern is broken"
    barred = {h for h in seen if h in ("mcpc_kernels.h", "mcpc_plan.h", "mcpc_hebbian.h", "mcpc_engine.h") or h.startswith("mcpc_steps_")}
    assert not barred, f"mcpc_records.hip includes {sorted(barred)}"
    # the object agrees: whatever it leaves undefined is the HIP runtime's and libc's, nothing of the library's other units
    run = subprocess.run(["nm", "-u", "-C", os.path.join(OBJDIR, "mcpc_records.o")], capture_output=True, text=True, check=True)
    ours = [line.strip() for line in run.stdout.splitlines() if "mcpc" in line]
    assert not ours, ours


def test_run_unit_sees_no_kernel_header(built):
    dep = open(os.path.join(OBJDIR, "mcpc_run.d")).read()
    seen = set(re.findall(r"(mcpc_\w+\.(?:h|inc))", dep))
    assert {"mcpc_engine.h", "mcpc_step_forms.h", "mcpc_plan.h"} <= seen, "the depfile does not name the unit's own headers: the pattern is broken"
    kernel_headers = {"mcpc_kernels.h", "mcpc_ws2_lean.h", "mcpc_ws2_fill.h", "mcpc_lw_tile.h", "mcpc_gemm_f16.h", "mcpc_step_math.h", "mcpc_engine_kernels.h",
                      "mcpc_chain_energy.h", "mcpc_pred_err.h", "mcpc_ancestral.h", "mcpc_hebbian.h",                                    # evaluators, Hebbian flush
                      "mcpc_moments.h", "mcpc_cov.h", "mcpc_hist.h", "mcpc_hist2d.h", "mcpc_acov.h", "mcpc_roll.h", "mcpc_probe.h", "mcpc_knn.h", "mcpc_loglik.h"}
    for h in kernel_headers:
        assert os.path.exists(os.path.join(CSRC, h)), f"{h} is no file of csrc/: the list is stale"
    barred = {h for h in seen if h in kernel_headers or h.startswith("mcpc_steps_")}
    assert not barred, f"mcpc_run.hip includes {sorted(barred)}"
    # the object agrees: of the library's other units it needs host functions -- the launchers among them -- and not one kernel's stub
    run = subprocess.run(["nm", "-u", "-C", os.path.join(OBJDIR, "mcpc_run.o")], capture_output=True, text=True, check=True)
    ours = [line.split(None, 1)[1].strip() for line in run.stdout.splitlines() if "mcpc" in line]
    launchers = ("mcpc::launch_ws2(", "mcpc::launch_u(", "mcpc::launch_barrier(", "mcpc::launch_lw_steps(", "mcpc::launch_lw_act(", "mcpc::launch_mu1(",
                 "mcpc::flush_spill(")
    for fn in launchers:
        assert any(sym.startswith(fn) for sym in ours), (fn, ours)
    stubs = [sym for sym in ours if "_kernel" in sym]
    assert not stubs, stubs


def planned(touched):
    """What `make` would do if `touched` were newer than everything: the units it recompiles, and whether it links."""
    run = subprocess.run(["make", "-C", CSRC, "-n", "-W", touched], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    units = set(re.findall(r"-c (mcpc_\w+)\.hip", run.stdout))
    assert units <= set(UNITS), units
    return units, "-shared" in run.stdout


@pytest.mark.parametrize("touched, units", [
    ("mcpc_hist.h", {"mcpc_records", "mcpc_build_info"}),
    ("mcpc_hebbian.h", {"mcpc_flush", "mcpc_build_info"}),
    ("mcpc_steps_u.h", {"mcpc_steps_u", "mcpc_build_info"}),
    ("mcpc_steps_ws2_body.inc", {"mcpc_steps_ws2", "mcpc_steps_ws2_spec", "mcpc_build_info"}),
    ("mcpc_chain_energy.h", {"mcpc_eval", "mcpc_build_info"}),
    ("mcpc_run.hip", {"mcpc_run", "mcpc_build_info"}),
])
def test_an_edit_recompiles_its_unit_and_the_build_info(built, touched, units):
    assert planned(touched) == (units, True)


def test_a_step_kernel_edit_leaves_the_records_unit_alone(built):
    units, links = planned("mcpc_gemm_f16.h")
    assert links and units == set(UNITS) - {"mcpc_run", "mcpc_records"}, units


def test_nothing_to_do_when_nothing_changed(built):
    run = subprocess.run(["make", "-C", CSRC, "-n"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    # (the two stamp recipes are printed -- they run under -n and rewrite nothing -- and nothing else)
    assert " -c " not in run.stdout and "-shared" not in run.stdout, run.stdout

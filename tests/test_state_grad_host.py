"""mcpc_state_gradients without a device: the kernels' resources (make asm), the header against the binding (a gcc probe of the
descriptor's layout), the fp64 bound of the GPU tests on every case, and the keyword's host checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import state_grad_cases as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mcpc.h")


# ---- 16. resources ------------------------------------------------------------------------------------------------------------------------
def test_state_gradient_kernels_keep_their_registers_and_stay_out_of_scratch(tmp_path):
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
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    text = open(asm).read()
    sgk = {k: v for k, v in usage.items() if "mcpc_grad_" in k}
    assert len(sgk) == 3, sorted(usage)
    for stem in ("mcpc_grad_prep_kernel", "mcpc_grad_fwd_kernel", "mcpc_grad_bwd_kernel"):
        assert sum(stem in k for k in sgk) == 1, sorted(sgk)
    for k, u in sgk.items():
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        body = text[text.index(f"\n{k}:"):]
        body = body[:body.index("s_endpgm")]
        assert not re.findall(r"^\s*scratch_(load|store)", body, flags=re.M), f"{k}: scratch instructions"
        assert not re.findall(r"\b(global|flat|buffer)_atomic", body), f"{k}: an atomic"
        if "prep" not in k:
            # the tile of the layer-wise launches: its GEMM, its LDS (plus the fp64 row sums in the forward kernel), its occupancy
            assert u["VGPRs"] + u["AGPRs"] <= 168 and u["Occupancy"] >= 3 and u["LDS Size"] <= 24 * 1024, (k, u)
            assert len(re.findall(r"v_mfma_f32_16x16x32[_a-z0-9]*f16", body)) > 0, f"{k}: no fp16 MFMA"
            assert not re.findall(r"v_mfma_f32_\d+x\d+x\d+_?f32\b", body), f"{k}: an fp32 MFMA -- a second arithmetic"
    # no new kernel carries a name the other resource tests count
    for k in sgk:
        assert not any(s in k for s in ("mcpc_ce_", "mcpc_steps_", "mcpc_heb7_kernel", "mcpc_lw_", "mcpc_pe_", "mcpc_sp_"))


def test_the_kernels_live_in_one_header_of_the_evaluator_unit():
    users = []
    for name in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, name), errors="replace").read()
        if re.search(r'#include\s+"mcpc_state_grad\.h"', src):
            users.append(name)
    assert users == ["mcpc_eval.hip"]


# ---- 17. header and binding ---------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds(tmp_path):
    from montecarlopredictivecoding_amd import _lib
    hdr = open(HEADER).read()
    assert re.search(r"#define MCPC_ABI_VERSION 4\b", hdr) and _lib.ABI_VERSION == 4
    m = re.search(r"int mcpc_state_gradients\(([^;]*)\);", hdr)
    assert m, "mcpc_state_gradients is not declared"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert params == ["mcpc_engine* e", "const mcpc_gradient_desc* d"]
    res, args = _lib.SYMBOLS["mcpc_state_gradients"]
    assert res is C.c_int and len(args) == 2 and args[0] is C.c_void_p and args[1]._type_ is _lib.GradientDesc
    # the ctypes struct against the C layout, by a gcc probe (the header stays a C11 header)
    fields = [f[0] for f in _lib.GradientDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("%zu\\n", sizeof(mcpc_gradient_desc));']
    lines += [f'printf("%s %zu\\n", "{f}", offsetof(mcpc_gradient_desc, {f}));' for f in fields]
    lines.append("return 0;}")
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(probe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert C.sizeof(_lib.GradientDesc) == int(out[0])
    seen = []
    for line in out[1:]:
        if line:
            name, off = line.split()
            assert getattr(_lib.GradientDesc, name).offset == int(off), name
            seen.append(name)
    assert seen == fields == ["inputs", "x", "n_rec", "loss_kind", "loss_var", "mask_start", "grad", "energies", "max_rows", "stream"]


def test_refusals_that_need_no_device():
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    d = _lib.GradientDesc()
    assert lib.mcpc_state_gradients(None, C.byref(d)) == -1 and b"state gradients: null engine" in lib.mcpc_last_error()
    assert lib.mcpc_state_gradients(None, None) == -1


# ---- 18. the bound of the GPU tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sg.NETS))
def test_the_bound_is_finite_and_positive_on_every_case(name):
    c = sg.NETS[name]
    want, bound = sg.reference(name)
    assert len(want) == len(bound) == len(c["sizes"])
    for l, (w, bnd) in enumerate(zip(want, bound)):
        assert w.shape == bnd.shape == (sg.N_REC, c["B"], c["sizes"][l])
        assert np.isfinite(w).all() and np.isfinite(bnd).all() and (bnd > 0).all()
        # a bound of rounding errors: far below the gradients it bounds
        assert bnd.max() < 1e-3 * np.abs(w).max()


def test_the_cases_cover_what_the_kernels_branch_on():
    n = sg.NETS
    assert set(sg.OWN) < set(n) and len(n) == 7
    assert n["ident_nohead"]["n_out"] == 0 and len(n["ident_nohead"]["sizes"]) == 2
    assert len(n["six_tanh"]["sizes"]) == 6 and all(16 <= s <= 48 for s in n["six_tanh"]["sizes"]) and len(set(sg.ecoef("six_tanh"))) > 1
    assert n["wide_under_small"]["sizes"][-1] == 784 and n["wide_under_small"]["n_out"] == 10 and n["wide_under_small"]["B"] == 16
    # both store paths: widths that are multiples of four and widths that are not
    widths = {s for c in n.values() for s in c["sizes"]}
    assert {33, 17, 37} <= widths and any(s % 4 == 0 for s in widths)


# ---- the keyword ---------------------------------------------------------------------------------------------------------------------------
def test_check_gradients():
    from montecarlopredictivecoding_amd import ais
    assert ais.check_gradients("run") == "run" and ais.check_gradients("run", "mala") == "run"
    assert ais.check_gradients("evaluator", "mala") == "evaluator"
    for bad in (None, "engine", 1, b"run"):
        with pytest.raises(ValueError, match="gradients"):
            ais.check_gradients(bad, "mala")
    with pytest.raises(ValueError, match="adjust"):
        ais.check_gradients("evaluator", None)

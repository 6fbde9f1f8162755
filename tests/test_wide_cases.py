"""CPU checks of the wide-network work (csrc/mcpc_steps_lw.h): the parity cases are parity cases, the two kernels keep their resources,
and the job tables of the two launches cover every tile once."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import wide_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_every_wide_case_is_a_parity_case(name):
    """The oracle in fp32 against the oracle in fp64: the reference's own rounding stays far inside the contract the GPU tests hold the
    engine to (states 1e-5, energies 1e-6, bucket 2e-4 / 2e-5 of its maximum).  A case that misses this (a ReLU kink that flips between
    the two precisions) is no parity case and is replaced in tests/wide_cases.py, never skipped."""
    case = wc.CASES[name]
    a, b = wc.oracle_run(case, np.float32), wc.oracle_run(case, np.float64)
    dx = max(float(np.abs(x - y).max()) for x, y in zip(a.xs, b.xs))
    de = float(np.max(np.abs(a.overall - b.overall) / np.abs(b.overall)))
    ga, gb = wc.bucket(a), wc.bucket(b)
    dg = float(np.abs(ga - gb).max() / np.abs(gb).max())
    print("%s: states %.2e  overall %.2e  bucket %.2e" % (name, dx, de, dg))
    assert dx <= 2e-6 and de <= 1e-7 and dg <= 1e-6, (name, dx, de, dg)


def test_the_table_holds_the_shapes_the_engine_tests_need():
    shapes = {(tuple(c["sizes"]), c["n_out"]) for c in wc.CASES.values()}
    for want in [((64, 1024, 1024), 0), ((32, 384), 100), ((512, 512), 10), ((30, 512, 512), 784), ((50, 700, 333), 1000)]:
        assert want in shapes
    assert any(len(c["sizes"]) == 6 for c in wc.CASES.values())
    assert all(n in wc.CASES for n in wc.REJECTED)


def test_layerwise_kernels_keep_their_registers_and_stay_out_of_scratch(tmp_path):
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
    text = open(asm).read()
    lw = {k: v for k, v in usage.items() if "mcpc_lw_fwd_kernel" in k or "mcpc_lw_bwd_kernel" in k}
    assert len(lw) == 2, sorted(usage)
    for k, u in lw.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (k, u)
        body = text[text.index(f"\n{k}:"):]
        body = body[:body.index("s_endpgm")]
        assert not re.findall(r"^\s*scratch_(load|store)", body, flags=re.M), f"{k}: scratch instructions"
        assert len(re.findall(r"v_mfma_f32_16x16x32[_a-z0-9]*f16", body)) > 0, f"{k}: no fp16 MFMA"
        assert not re.findall(r"v_mfma_f32_\d+x\d+x\d+_?f32\b", body), f"{k}: an fp32 MFMA -- a second arithmetic"
    # no new kernel carries a name tests/test_build_info.py counts
    for k in usage:
        if "mcpc_lw_" in k:
            assert not any(s in k for s in ("mcpc_steps_u_kernel", "mcpc_steps_ws2_kernelILi1E", "mcpc_heb7_kernel"))
    assert len([k for k in usage if "mcpc_steps_ws2_kernelILi1E" in k]) == 2
    assert len([k for k in usage if "mcpc_steps_u_kernel" in k]) == 2
    assert len([k for k in usage if "mcpc_heb7_kernel" in k]) >= 6


def _jobs(sizes, n_out):
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    cap = 4096
    fwd, bwd = (C.c_int32 * (2 * cap))(), (C.c_int32 * (2 * cap))()
    nf, nb, tile = C.c_int32(), C.c_int32(), (C.c_int32 * 2)()
    arr = (C.c_int32 * len(sizes))(*sizes)
    _lib.check(lib.mcpc_debug_lw_jobs(len(sizes), arr, n_out, fwd, bwd, cap, C.byref(nf), C.byref(nb), tile))
    assert nf.value <= cap and nb.value <= cap
    return ([(fwd[2 * i], fwd[2 * i + 1]) for i in range(nf.value)], [(bwd[2 * i], bwd[2 * i + 1]) for i in range(nb.value)], tile[0], tile[1])


@pytest.mark.parametrize("sizes,n_out", [([200, 33, 17], 1000), ([1000], 0), ([17], 1), ([33, 200, 384], 100), ([64, 1024, 1024], 0),
                                        ([30, 512, 512], 784), ([320] * 6, 5), ([1, 2049], 4097)])
def test_job_tables_cover_every_tile_once(sizes, n_out):
    fwd, bwd, chains, unit_tiles = _jobs(sizes, n_out)
    assert 32 <= chains <= 64 and 64 <= 16 * unit_tiles <= 128
    L_ = len(sizes)
    tiles = lambda n: (n + 15) // 16

    def covered(jobs, layers):
        seen = {}
        for layer, ut0 in jobs:
            assert layer in layers and ut0 % unit_tiles == 0, (layer, ut0)
            for ut in range(ut0, min(ut0 + unit_tiles, layers[layer])):
                seen[(layer, ut)] = seen.get((layer, ut), 0) + 1
        want = {(l, ut) for l, n in layers.items() for ut in range(n)}
        assert set(seen) == want and all(v == 1 for v in seen.values()), (sorted(set(seen) ^ want)[:5])
        assert all(ut0 < layers[layer] for layer, ut0 in jobs)          # no job without a tile

    f_layers = {l: tiles(n) for l, n in enumerate(sizes)}
    if n_out:
        f_layers[L_] = tiles(n_out)
    covered(fwd, f_layers)
    covered(bwd, {l: tiles(n) for l, n in enumerate(sizes)})


def test_wide_keys_parse_without_a_device():
    """What can be said of the two keys without a GPU: the header documents them and the ABI did not move."""
    hdr = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert "wide=1" in hdr and "ws=0|2|3|4" in hdr and "mcpc_lw_fwd_kernel" in hdr
    assert re.search(r"#define MCPC_ABI_VERSION 4\b", hdr)

"""CPU checks of the per-chain energy evaluator (csrc/mcpc_chain_energy.h): the request is validated, the job table covers every
tile once with each Linear's jobs in the order they are added, the kernels keep their registers, and the header declares what the
binding binds."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")


def test_spec_validation():
    from montecarlopredictivecoding_amd.chain_energies import sample_steps, validate_spec
    s = validate_spec(dict(begin=2, stride=3), 12)
    assert (s.begin, s.stride, s.T, s.n, s.steps) == (2, 3, 12, 4, [2, 5, 8, 11])
    d = validate_spec({}, 5)
    assert (d.begin, d.stride, d.n) == (0, 1, 5) and list(sample_steps(0, 5, 1)) == d.steps
    assert validate_spec(dict(begin=4), 5).steps == [4]
    for bad, word in ((dict(layers=(0,)), "unknown keys"), (dict(begin=12), "begin=12"), (dict(begin=-1), "begin=-1"),
                      (dict(stride=0), "stride=0"), (dict(stride=-2), "stride=-2"), (dict(begin=1.0), "begin must be an int"),
                      (dict(stride=True), "stride must be an int"), ([0, 1], "expected a dict")):
        with pytest.raises(ValueError, match=word):
            validate_spec(bad, 12)
    # the samples of a slice: rows of a chunk that holds one record per step from t0 on
    for t0, n, want in ((0, 2, (2, 0)), (0, 3, (2, 1)), (2, 4, (0, 2)), (3, 3, (2, 1)), (6, 6, (2, 2)), (9, 3, (2, 1)), (9, 2, (2, 0))):
        assert s.chunk(t0, n) == want, (t0, n)
    seen = []
    for t0, n in ((0, 5), (5, 1), (6, 6)):
        first, cnt = s.chunk(t0, n)
        seen += [t0 + first + k * s.stride for k in range(cnt)]
    assert seen == s.steps


def test_trainer_carries_the_request_and_refuses_a_bad_one_before_any_work():
    import torch
    import montecarlopredictivecoding_amd.predictive_coding as pc
    m = torch.nn.Sequential(torch.nn.Linear(3, 3), pc.PCLayer(), torch.nn.Linear(3, 2))
    m.train()
    tr = pc.PCTrainer(m, T=3, update_p_at="never", plot_progress_at=[])
    assert tr.mcpc_chain_energies is None and tr.mcpc_last_chain_energies is None and callable(tr.mcpc_state_energies)
    from montecarlopredictivecoding_amd.utils import training_evaluation as te
    assert callable(te.get_map_free_energy)
    with pytest.raises(AttributeError):
        te.get_fid_of_no_script


def _jobs(sizes, n_out):
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    cap = 4096
    jobs = (C.c_int32 * (2 * cap))()
    n, nh, tile = C.c_int32(), C.c_int32(), (C.c_int32 * 2)()
    arr = (C.c_int32 * len(sizes))(*sizes)
    _lib.check(lib.mcpc_debug_chain_energy_jobs(len(sizes), arr, n_out, jobs, cap, C.byref(n), C.byref(nh), tile))
    assert n.value <= cap
    return [(jobs[2 * i], jobs[2 * i + 1]) for i in range(n.value)], nh.value, tile[0], tile[1]


@pytest.mark.parametrize("sizes,n_out", [([6, 16, 16], 24), ([200, 33, 17], 40), ([272, 144], 784), ([37], 0), ([200, 33, 17], 1000),
                                        ([1000], 0), ([17], 1), ([320] * 6, 5), ([1, 2049], 4097)])
def test_job_table_covers_every_tile_once(sizes, n_out):
    jobs, n_head, rows, unit_tiles = _jobs(sizes, n_out)
    assert rows == 64 and unit_tiles == 8
    L_ = len(sizes)
    tiles = lambda n: (n + 15) // 16
    layers = {l: tiles(n) for l, n in enumerate(sizes)}
    if n_out:
        layers[L_] = tiles(n_out)
    seen = {}
    for layer, ut0 in jobs:
        assert layer in layers and ut0 % unit_tiles == 0 and ut0 < layers[layer], (layer, ut0)
        for ut in range(ut0, min(ut0 + unit_tiles, layers[layer])):
            seen[(layer, ut)] = seen.get((layer, ut), 0) + 1
    want = {(l, ut) for l, n in layers.items() for ut in range(n)}
    assert set(seen) == want and all(v == 1 for v in seen.values())
    # the read-out's jobs are the first n_head (a call without a loss launches the rest); a Linear's jobs are contiguous and ascending
    assert [j for j in jobs[:n_head]] == [(L_, ut) for ut in range(0, tiles(n_out), unit_tiles)]
    assert all(layer < L_ for layer, _ in jobs[n_head:])
    order = [layer for layer, _ in jobs]
    for l in layers:
        idx = [i for i, x in enumerate(order) if x == l]
        assert idx == list(range(idx[0], idx[0] + len(idx)))
        assert [jobs[i][1] for i in idx] == sorted(jobs[i][1] for i in idx)


def test_job_table_rejects_a_bad_network():
    from montecarlopredictivecoding_amd import _lib
    lib = _lib.load()
    n = C.c_int32()
    assert lib.mcpc_debug_chain_energy_jobs(0, (C.c_int32 * 1)(4), 0, None, 0, C.byref(n), None, None) == -1
    assert lib.mcpc_debug_chain_energy_jobs(1, (C.c_int32 * 1)(0), 0, None, 0, C.byref(n), None, None) == -1
    assert lib.mcpc_debug_chain_energy_jobs(1, (C.c_int32 * 1)(4), 0, None, 0, C.byref(n), None, None) == 0 and n.value == 1


def test_chain_energy_kernels_keep_their_registers_and_stay_out_of_scratch(tmp_path):
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
    ce = {k: v for k, v in usage.items() if "mcpc_ce_" in k}
    assert len(ce) == 3 and sum("mcpc_ce_kernel" in k for k in ce) == 1, sorted(usage)
    for k, u in ce.items():
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        body = text[text.index(f"\n{k}:"):]
        body = body[:body.index("s_endpgm")]
        assert not re.findall(r"^\s*scratch_(load|store)", body, flags=re.M), f"{k}: scratch instructions"
        assert not re.findall(r"\b(global|flat|buffer)_atomic", body), f"{k}: an atomic"
        if "mcpc_ce_kernel" in k:
            # the tile of the layer-wise forward launch: its GEMM, its LDS plus the fp64 row sums, at least its occupancy
            assert u["VGPRs"] + u["AGPRs"] <= 168 and u["Occupancy"] >= 3 and u["LDS Size"] <= 24 * 1024, (k, u)
            assert len(re.findall(r"v_mfma_f32_16x16x32[_a-z0-9]*f16", body)) > 0, f"{k}: no fp16 MFMA"
            assert not re.findall(r"v_mfma_f32_\d+x\d+x\d+_?f32\b", body), f"{k}: an fp32 MFMA -- a second arithmetic"
    # no new kernel carries a name the other resource tests count
    for k in ce:
        assert not any(s in k for s in ("mcpc_steps_u_kernel", "mcpc_steps_ws2_kernel", "mcpc_heb7_kernel", "mcpc_lw_"))


def test_header_declares_what_the_binding_binds():
    from montecarlopredictivecoding_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"#define MCPC_ABI_VERSION 4\b", hdr)
    m = re.search(r"int mcpc_chain_energies\(([^;]*)\);", hdr)
    assert m, "mcpc_chain_energies is not declared"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert len(params) == len(_lib.SYMBOLS["mcpc_chain_energies"][1]) == 10
    assert params[0].startswith("mcpc_engine*") and params[1] == "const float* inputs" and params[2] == "const float* const* x_rec"
    assert params[3] == "int32_t n_rec" and params[5] == "double loss_var" and params[7] == "double* out" and params[8] == "int32_t max_rows"
    assert _lib.SYMBOLS["mcpc_chain_energies"][1][5] is C.c_double
    m = re.search(r"int mcpc_debug_chain_energy_jobs\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == len(_lib.SYMBOLS["mcpc_debug_chain_energy_jobs"][1]) == 8
    assert callable(getattr(_lib.load(), "mcpc_chain_energies"))

"""Posterior moments, host side (no GPU): the `mcpc_moments` request, the sample count, the C entry point's declaration and binding,
and the registers of the reduction kernel."""
import os
import re
import subprocess

import pytest
import torch

from montecarlopredictivecoding_amd import _lib
from montecarlopredictivecoding_amd import moments as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")


@pytest.mark.parametrize("spec, word", [
    (dict(begin=5, strid=2), "unknown keys"),
    (dict(begin=-1), "begin"),
    (dict(begin=60), "begin"),
    (dict(stride=0), "stride"),
    (dict(layers=(0, 3)), "layer index"),
    (dict(layers=(-1,)), "layer index"),
    (dict(outputs="softmax"), "outputs"),
])
def test_invalid_requests_are_value_errors(spec, word):
    with pytest.raises(ValueError, match=word):
        M.validate_spec(spec, T=60, n_layers=3, n_out=24)


def test_outputs_need_a_read_out():
    with pytest.raises(ValueError, match="read-out"):
        M.validate_spec(dict(outputs="identity"), T=60, n_layers=2, n_out=0)
    assert M.validate_spec(dict(layers=(1,)), T=60, n_layers=2, n_out=0).layers == (1,)


def test_the_trainer_has_the_opt_in_attributes_and_they_are_off():
    import montecarlopredictivecoding_amd.predictive_coding as pc
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), pc.PCLayer(), torch.nn.Linear(2, 3))
    tr = pc.PCTrainer(model, T=4, plot_progress_at=[])
    assert tr.mcpc_moments is None and tr.mcpc_last_moments is None and tr.mcpc_moments_chunk_bytes > 0


@pytest.mark.parametrize("begin, stride, T", [(0, 1, 1), (20, 3, 60), (59, 7, 60), (200, 1, 1000), (3, 4, 5), (0, 60, 60)])
def test_sample_count_and_chunks(begin, stride, T):
    spec = M.validate_spec(dict(begin=begin, stride=stride), T=T, n_layers=1, n_out=0)
    steps = list(range(begin, T, stride))
    assert spec.n == len(steps)
    for S in (1, 5, 7, T):                               # however the call is sliced, the chunks name exactly the sample steps
        got = []
        for t0 in range(0, T, S):
            n = min(S, T - t0)
            first, cnt = spec.chunk(t0, n)
            assert cnt == 0 or (0 <= first and first + (cnt - 1) * stride < n)
            got += [t0 + first + k * stride for k in range(cnt)]
        assert got == steps


def test_mean_and_variance_from_sums():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(9, 5, generator=g, dtype=torch.float64)
    s, q = v.sum(0), (v * v).sum(0)
    m = M.Moments(n=9, x_sum=[s, None], x_sumsq=[q, None])
    assert m.x_mean[1] is None and m.x_var[1] is None and m.out_mean is None and m.out_var is None
    assert m.x_mean[0].dtype == torch.float32 and torch.equal(m.x_mean[0], (s / 9).float())
    torch.testing.assert_close(m.x_var[0], v.var(0, unbiased=True).float(), rtol=1e-6, atol=0)
    one = M.Moments(n=1, x_sum=[v[0]], x_sumsq=[v[0] * v[0]])
    assert torch.isnan(one.x_var[0]).all()
    assert M.Moments(n=9, x_sum=[s], x_sumsq=[None]).x_var[0] is None          # variance=False: no sumsq, no variance
    both = m.merge(m)
    assert both.n == 18 and torch.equal(both.x_sum[0], s + s) and both.x_sum[1] is None


def test_header_declares_the_entry_point_and_the_binding_binds_it():
    header = open(os.path.join(ROOT, "include", "mcpc.h")).read()
    assert re.search(r"\bint\s+mcpc_moments_accumulate\s*\(", header)
    assert re.search(r"#define\s+MCPC_MOM_IDENTITY\s+0\b", header) and re.search(r"#define\s+MCPC_MOM_SIGMOID\s+1\b", header)
    assert re.search(r"#define\s+MCPC_ABI_VERSION\s+4\b", header)
    res, args = _lib.SYMBOLS["mcpc_moments_accumulate"]
    assert len(args) == 11
    assert (_lib.MOM_IDENTITY, _lib.MOM_SIGMOID) == (0, 1)


def test_moments_kernel_keeps_its_registers_and_stays_out_of_scratch(tmp_path):
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
    mom = {k: v for k, v in usage.items() if "mcpc_moments_kernel" in k}
    assert len(mom) == 8, sorted(usage)                    # {16-B, scalar} x {identity, sigmoid} x {with, without sumsq}
    for k, u in mom.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)

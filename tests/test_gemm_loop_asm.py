"""The instruction stream of the GEMM waves' steady-state loop in the specialised step kernels, read from `make asm` (CPU suite).

A GEMM wave shares its SIMD with an epilogue wave, and beside a 16x16x32 MFMA every other vector instruction of the loop costs its
issue time, so what the loop carries besides its MFMAs is held here, per specialised instantiation of
mcpc_steps_ws2_spec_kernel, on the basic block that is the rotation's period -- three k-blocks of four tiles: 36 MFMAs and 24 fragment
loads (csrc/mcpc_gemm_f16.h: gemm_fixed):

* the operand split's second piece is one v_fma_mixlo_f16 / v_fma_mixhi_f16 per value (24 per block) and nothing converts fp16 back
  to fp32 (split2_pair);
* every fragment load has a scalar base and one 32-bit lane offset (`global_load_dwordx4 v[..], v_off, s[b:b+1] offset:..`): no 64-bit
  VALU address arithmetic in the loop (load_frag_at);
* at most 60 vector-ALU instructions that are not MFMAs (101 before the two changes; 8 values take 4 products, 4 conversions and 8
  fmas = 16 per k-block = 48, plus the B rows' LDS addresses: profiles/gemm_diet_asm.txt has the listings).

A subnormal second piece needs the kernels to keep denormals: every kernel descriptor of the unit says so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")
UNITS = "mcpc_steps_ws2_spec mcpc_steps_u"


@pytest.fixture(scope="module")
def spec_asm(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("asm") / "spec.s")
    run = subprocess.run(["make", "-C", CSRC, "asm", f"KERNEL_UNITS={UNITS}", f"ASM_OUT={asm}"], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    return open(asm).read()


def _kernels(text):
    """name -> body of every specialised instantiation"""
    out = {}
    for m in re.finditer(r"^(_ZN4mcpc26mcpc_steps_ws2_spec_kernel\w+):[^\n]*\n", text, flags=re.M):
        body = text[m.end():]
        out[m.group(1)] = body[:body.index("s_endpgm")]
    return out


def _basic_blocks(body):
    """instructions of each basic block: cut at labels and behind branches"""
    blocks, cur = [], []
    for line in body.splitlines():
        s = line.split(";")[0].strip()
        if not s:
            continue
        if re.match(r"\.?\w+:$", s):
            blocks.append(cur)
            cur = []
            continue
        if s.startswith("."):
            continue
        cur.append(s)
        if re.match(r"s_c?branch", s) or s.startswith("s_setpc"):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    return [b for b in blocks if b]


def _steady_state_blocks(body):
    return [b for b in _basic_blocks(body)
            if sum(i.startswith("v_mfma_f32_16x16x32_f16") for i in b) == 36
            and sum(bool(re.match(r"(global|buffer)_load_dwordx4\b", i)) for i in b) == 24]


def test_there_are_six_specialised_instantiations_each_with_the_loop(spec_asm):
    kernels = _kernels(spec_asm)
    assert len(kernels) == 6, sorted(kernels)
    for name, body in kernels.items():
        assert _steady_state_blocks(body), f"{name}: no basic block with 36 MFMAs and 24 fragment loads"


def test_second_piece_is_one_mixed_precision_fma_per_value(spec_asm):
    for name, body in _kernels(spec_asm).items():
        for b in _steady_state_blocks(body):
            mix = [i for i in b if re.match(r"v_fma_mix(lo|hi)_f16\b", i)]
            assert len(mix) == 24, (name, len(mix))
            assert sum(i.startswith("v_fma_mixlo_f16") for i in mix) == 12, name
            assert not [i for i in b if i.startswith("v_cvt_f32_f16")], name
            # the residual is x s - h: the fp16 operand is the one subtracted
            assert all(re.search(r", -v\d+ ", i + " ") for i in mix), (name, mix[:2])


def test_fragment_loads_take_a_scalar_base_and_one_lane_offset(spec_asm):
    for name, body in _kernels(spec_asm).items():
        for b in _steady_state_blocks(body):
            assert not [i for i in b if i.startswith("v_lshl_add_u64") or i.startswith("v_addc_co_u32")], name
            loads = [i for i in b if i.startswith("global_load_dwordx4")]
            assert len(loads) == 24, (name, len(loads))
            for i in loads:
                assert re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]( offset:-?\d+)?$", i), (name, i)
            # the k advance is the scalar ALU's: the base pair every load names is stepped by one s_add_u32 / s_addc_u32 in the block
            bases = {re.search(r"s\[(\d+):(\d+)\]", i).groups() for i in loads}
            assert len(bases) == 1, (name, bases)
            lo, hi = bases.pop()
            assert sum(bool(re.match(rf"s_add_u32 s{lo}, s{lo}, ", i)) for i in b) == 1, (name, lo)
            assert sum(bool(re.match(rf"s_addc_u32 s{hi}, s{hi}, ", i)) for i in b) == 1, (name, hi)
            assert sum(i.startswith("s_add_u32") for i in b) <= 2 and sum(i.startswith("s_addc_u32") for i in b) <= 2, name


def test_unified_wave_kernel_streams_its_fragments_the_same_way(spec_asm):
    """gemm_deep (one or two tiles per wave) and gemm_fixed inside mcpc_steps_u_kernel: every basic block that streams fragments beside
    MFMAs -- at least 12 MFMAs and 6 fragment loads -- loads them with a scalar base and has the single-rounding split.  (The prefetch
    of an entry's first blocks, load_frag, sits among the epilogue's other global loads and is not told apart here.)"""
    kernels = {m.group(1): spec_asm[m.end():] for m in re.finditer(r"^(_ZN4mcpc19mcpc_steps_u_kernel\w+):[^\n]*\n", spec_asm, flags=re.M)}
    assert len(kernels) == 2, sorted(kernels)
    for name, body in kernels.items():
        blocks = [b for b in _basic_blocks(body[:body.index("s_endpgm")])
                  if sum(i.startswith("v_mfma_f32_16x16x32_f16") for i in b) >= 12 and sum(i.startswith("global_load_dwordx4") for i in b) >= 6]
        assert len(blocks) >= 4, (name, len(blocks))
        for b in blocks:
            assert not [i for i in b if i.startswith("v_lshl_add_u64") or i.startswith("v_addc_co_u32") or i.startswith("v_cvt_f32_f16")], name
            for i in b:
                if i.startswith("global_load_dwordx4"):
                    assert re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]( offset:-?\d+)?$", i), (name, i)


def test_loop_carries_at_most_sixty_other_vector_alu_instructions(spec_asm):
    for name, body in _kernels(spec_asm).items():
        for b in _steady_state_blocks(body):
            valu = [i for i in b if i.startswith("v_") and not i.startswith("v_mfma")]
            print(f"[gemm loop] {name[-52:]}: {len(b)} instructions, {len(valu)} VALU besides 36 MFMAs")
            assert len(valu) <= 60, (name, len(valu))


def test_kernels_keep_denormals(spec_asm):
    d32 = re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", spec_asm)
    d16 = re.findall(r"\.amdhsa_float_denorm_mode_16_64 (\d+)", spec_asm)
    assert len(d32) == len(d16) >= 8 and set(d32) == {"3"} and set(d16) == {"3"}, (d32, d16)

"""The step kernels' per-element arithmetic has ONE definition: csrc/mcpc_step_math.h.

Barrier, in-place, unified-wave and layer-wise kernels must produce the same trajectories bit for bit (the GPU suite asserts it);
they do so because their epilogues call the float4 helpers of that header instead of carrying copies.  The scalar building blocks
(Adam's three forms, the activation derivative, the sigmoid with and without the BCE term) are defined in csrc/mcpc_device.h and
may be CALLED from the header only.  `act_f` / `act_d`, the run-time forms (mcpc_lw_act_kernel), are not meant."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlopredictivecoding_amd", "csrc")
HOME = ("mcpc_step_math.h", "mcpc_device.h")
# a call or an instantiation; the \b keeps act_d( / bernoulli_mean( and the like out
SCALAR_FORMS = [r"\badam_m\(", r"\badam_v\(", r"\badam_x\(", r"\bactd<", r"\bsigmoid_bce_f\(", r"\bsigmoid_f\("]


def _code(path):
    """the file without its // comments (they may name the functions)"""
    return "\n".join(line.split("//", 1)[0] for line in open(path, errors="replace"))


def test_step_arithmetic_is_called_from_one_header_only():
    header = _code(os.path.join(CSRC, "mcpc_step_math.h"))
    for pat in SCALAR_FORMS:
        assert re.search(pat, header), f"the scan for {pat!r} found nothing in mcpc_step_math.h: the pattern is broken"
    scanned, strays = 0, []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        name = os.path.basename(path)
        if name in HOME or not os.path.isfile(path):
            continue
        scanned += 1
        code = _code(path)
        strays += [f"{name}: {m.group(0)}" for pat in SCALAR_FORMS for m in re.finditer(pat, code)]
    assert scanned >= 10, "the scan saw hardly any file of csrc/"
    assert not strays, f"step arithmetic outside csrc/mcpc_step_math.h: {strays}"

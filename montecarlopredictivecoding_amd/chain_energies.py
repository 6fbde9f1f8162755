"""Per-chain energies of a Langevin call: the request (``PCTrainer.mcpc_chain_energies``) and the result
(``PCTrainer.mcpc_last_chain_energies``, ``PCTrainer.mcpc_state_energies``).

The reference reports energies per datapoint behind ``is_return_batchelement_loss``, ``PCLayer(is_keep_energy_per_datapoint=True)`` and
``get_energies(is_per_datapoint=True)``; here a fused call evaluates them on the device out of its record ring
(csrc/mcpc_chain_energy.h) and the trajectory is never materialised.  This module holds no device code: validation of the request,
which steps are evaluated, and the split of the library's ``[n, B, L + 2]`` table into the three tensors a caller reads.
"""
from dataclasses import dataclass
from typing import List

import torch

from .sampling import SampleWindow, parse_keys, parse_window, sample_steps  # noqa: F401

_KEYS = ("begin", "stride")


@dataclass(frozen=True)
class ChainEnergySpec(SampleWindow):
    """A validated ``mcpc_chain_energies`` request for a call of ``T`` steps: the samples are the steps whose states are evaluated."""


def validate_spec(spec, T: int) -> ChainEnergySpec:
    """``PCTrainer.mcpc_chain_energies`` -> ChainEnergySpec, or ValueError: not a dict, unknown keys, ``begin`` outside [0, T),
    ``stride`` < 1.  Defaults: begin=0, stride=1."""
    parse_keys("mcpc_chain_energies", spec, _KEYS)
    begin, stride = parse_window("mcpc_chain_energies", spec, T)
    return ChainEnergySpec(begin=begin, stride=stride, T=T)


@dataclass
class ChainEnergies:
    """Energies of ``n`` states of ``B`` chains, fp64, on the model's device.  ``steps[k]`` is the step of the call whose forward saw
    state k (empty for ``mcpc_state_energies``).  ``loss [n, B]``, ``energy [n, B, L]`` (divided by the trainer's
    ``energy_coefficient``, as ``results["energy"]`` is), ``overall [n, B]``: summed over the chains they are the call's own results at
    those steps.  A staged (CPU) model gets them on the CPU; a sharded trainer sees its local chains only, in local order."""
    steps: List[int]
    loss: torch.Tensor
    energy: torch.Tensor
    overall: torch.Tensor


def from_table(table: torch.Tensor, n_layers: int, energy_coefficient: float, steps, device) -> ChainEnergies:
    """The library's ``[n, B, L_max + 2]`` table (loss, E_1.., overall) -> ChainEnergies on ``device``."""
    table = table.to(device)
    return ChainEnergies(steps=list(steps), loss=table[:, :, 0].contiguous(),
                         energy=(table[:, :, 1:1 + n_layers] / energy_coefficient).contiguous(),
                         overall=table[:, :, -1].contiguous())

"""Posterior covariances on the device, pinned by the reference: the three g13 cases of tests/test_gpu_sampling.py (stationary means and
the full 38 x 38 covariance of the concatenated latents, from the imported reference for 12 torch seeds) with the same seed and run
arguments but WITHOUT a recorded trajectory: the records go to a ring of a few hundred steps and `cov_accumulate` /
`moments_accumulate` reduce it between the slices of the run, pooled over the 4096 chains.  The criteria are that test's, unchanged:
every entry inside 8 spreads of a further reference seed, each group's mean square no further out than reference seeds are from each
other, the variances within 2 %."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.cases import make_case_inputs
from tests.test_gpu_sampling import _t_moments, _z

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLICE = 250                                                  # steps per slice: the ring holds 250 x 4096 x 38 floats, 156 MB


@pytest.mark.parametrize("name", ["tanh_gaussian", "relu_bernoulli", "relu_zero"])
def test_device_covariance_sits_inside_the_reference_seed_spread(name):
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.covariance import Covariance
    from montecarlopredictivecoding_amd.engine import Engine, cov_accumulate, cov_workspace_bytes, moments_accumulate
    g = np.load(os.path.join(GOLDEN, f"g13_sampling_moments_{name}.npz"))
    case = json.loads(str(g["case_json"]))
    burn, T, lr, nvar = int(g["burn"]), int(g["T"]), float(g["lr"]), float(g["noise_var"])
    W, b, X0, inputs, target = make_case_inputs(case)
    sizes, B, n_out = case["sizes"], case["B"], case["n_out"]
    act = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU}[case["acts"][0]]
    eng = Engine(sizes, [act] * 3, case["n_in"], n_out, B, device=DEV)
    eng.bind_params([torch.from_numpy(w).to(DEV) for w in W], [torch.from_numpy(v).to(DEV) for v in b])
    eng.bind_inputs(None)
    if target is not None:
        eng.bind_target(torch.from_numpy(target).to(DEV))
    eng.load_state([torch.from_numpy(x).to(DEV) for x in X0])
    kind = {"gaussian": L.LOSS_GAUSSIAN, "bernoulli": L.LOSS_BERNOULLI, "zero": L.LOSS_NONE}[case["loss"]]
    gen = case["loss"] == "zero"
    D = sum(sizes)
    ring = [torch.empty(SLICE, B, n, dtype=torch.float32, device=DEV) for n in sizes]
    ring_o = torch.empty(SLICE, B, n_out, dtype=torch.float32, device=DEV) if gen else None
    sums = [torch.zeros(B, n, dtype=torch.float64, device=DEV) for n in sizes]
    outer = torch.zeros(D, D, dtype=torch.float64, device=DEV)
    ws = torch.empty(cov_workspace_bytes(B, sizes), dtype=torch.uint8, device=DEV)
    if gen:
        out_sum = torch.zeros(B, n_out, dtype=torch.float64, device=DEV)
        out_outer = torch.zeros(n_out, n_out, dtype=torch.float64, device=DEV)
        ws_o = torch.empty(cov_workspace_bytes(B, [n_out]), dtype=torch.uint8, device=DEV)
    energies = torch.zeros(T, L.ENERGY_COLS, dtype=torch.float64, device=DEV)
    slices = 0
    for t0 in range(0, T, SLICE):
        n = min(SLICE, T - t0)
        eng.run(T, t_begin=t0, n_steps=n, adam_step0=t0, energies_out=energies, loss_kind=kind, loss_var=case["var"], xopt=L.XOPT_SGD,
                lr=lr, noise_mode=L.NOISE_PHILOX, noise_var=nvar, seed=20260104, step_base=0, energy_mode=L.ENERGY_ALL,
                rec_begin=t0, rec_stride=1, rec_count=n, rec_x=True, rec_x_bufs=ring, rec_out=gen, rec_out_buf=ring_o)
        first = max(burn - t0, 0)
        if first < n:
            for r, s in zip(ring, sums):
                moments_accumulate(r, first, 1, n - first, s, None, accumulate=True)
            cov_accumulate(ring, first, 1, n - first, outer, pool=True, accumulate=True, workspace=ws)
            if gen:
                moments_accumulate(ring_o, first, 1, n - first, out_sum, None, accumulate=True)
                cov_accumulate([ring_o], first, 1, n - first, out_outer, pool=True, accumulate=True, workspace=ws_o)
        slices += 1
    eng.sync_check()
    assert slices == T // SLICE and T % SLICE == 0
    columns, start = [], 0
    for l, w in enumerate(sizes):
        columns.append((f"x{l}", start, w))
        start += w
    c = Covariance(n=T - burn, B=B, pooled=True, columns=columns, sum=torch.cat(sums, dim=1).sum(0), outer=outer)
    mean, cov = c.mean.cpu().numpy(), c.cov(ddof=0).cpu().numpy()
    assert np.array_equal(cov, cov.T)
    if gen:
        co = Covariance(n=T - burn, B=B, pooled=True, columns=[("out", 0, n_out)], sum=out_sum.sum(0), outer=out_outer)
        out_mean, out_cov = co.mean.cpu().numpy(), co.cov(ddof=0).cpu().numpy()
    en = energies.cpu().numpy()[burn:]
    en3 = np.array([en[:, 0].mean(), en[:, 1:4].sum(1).mean(), en[:, -1].mean()])
    eng.close()

    n_seeds = g["mean"].shape[0]
    m2, v2 = _t_moments(n_seeds - 1)
    iu = np.triu_indices(cov.shape[0], k=1)
    groups = {"means": _z(mean, g["mean"]),
              "variances": _z(np.diag(cov), np.array([np.diag(c_) for c_ in g["cov"]])),
              "covariances": _z(cov[iu], np.array([c_[iu] for c_ in g["cov"]])),
              "energies": _z(en3[1:] if gen else en3, g["energies"][:, 1:] if gen else g["energies"])}
    if gen:
        ju = np.triu_indices(out_cov.shape[0], k=1)
        groups["read-out means"] = _z(out_mean, g["out_mean"])
        groups["read-out variances"] = _z(np.diag(out_cov), np.array([np.diag(c_) for c_ in g["out_cov"]]))
        groups["read-out covariances"] = _z(out_cov[ju], np.array([c_[ju] for c_ in g["out_cov"]]))
    for key, z in groups.items():
        print(f"{name}, {key}: max |z| {float(np.abs(z).max()):.2f}, mean z^2 {float((z * z).mean()):.2f}")
        assert np.abs(z).max() < 8.0, (key, float(np.abs(z).max()))
        assert (z * z).mean() < m2 + 5.0 * np.sqrt(v2 / z.size), (key, float((z * z).mean()))
    np.testing.assert_allclose(np.diag(cov), np.array([np.diag(c_) for c_ in g["cov"]]).mean(0), rtol=2e-2)
    if gen:
        np.testing.assert_allclose(np.diag(out_cov), np.array([np.diag(c_) for c_ in g["out_cov"]]).mean(0), rtol=2e-2)

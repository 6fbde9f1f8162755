"""The fused sampler's normals over Box-Muller's whole domain (csrc/mcpc_device.h: box_muller; include/mcpc.h: mcpc_box_muller) against
the float64 definition and the bounds of tests/box_muller_cases.py.

The transform is separable and each factor has 2^24 arguments (the low 8 bits of either Philox word are shifted out), so
  a. every radius is compared with fp64 under the derived relative bound, with no NaN, no negative value, a zero at u1 = 1 and the
     design limit sqrt(48 ln 2) as the tail;
  b. every angle, at the largest radius, a middle one and one next to u1 = 1, keeps a normal within 2e-5 of fp64 and inside the radius;
  c. the moments of the device's distribution over the full 2^24 x 2^24 grid, exact products of table means, are inside caps that no
     sampled statistic could resolve;
  d. the diagnostic entry applied to the raw Philox words is bitwise the normals `mcpc_philox_normals` reports;
  e. every step-kernel form applies exactly these normals: with all weights zero, lr = 1 and a kick scale of exactly 0.5 the state after
     step t is 0.5 z(seed, step_base + t, layer, chain, unit), also where the step counter crosses 2^32, where the u32 chain id wraps
     inside the batch, with a 64-bit seed and with the call cut into slices.
The worst errors of a-c are printed ([box-muller] lines: run with -s) and recorded in profiles/box_muller_accuracy.txt; the angle
functions' errors are measurements, not bounds."""
import numpy as np
import pytest
import torch

from oracle import philox
from tests import box_muller_cases as bm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = bm.N
A_MID = np.uint32(0x7FFFFF00)                       # u1 = 1/2
A_NEAR_ONE = np.uint32((N - 9) << 8)                # u1 = 1 - 2^-21
QUARTERS = np.uint32([0, 0x40000000, 0x80000000, 0xC0000000])


def _say(msg):
    print("[box-muller] " + msg)


def _device(a, b):
    """(z0, z1) of the device's transform of two uint32 arrays, as float32 NumPy arrays."""
    from montecarlopredictivecoding_amd.engine import box_muller
    shape = np.broadcast_shapes(np.shape(a), np.shape(b))
    a, b = (np.array(np.broadcast_to(np.asarray(x, dtype=np.uint32), shape)) for x in (a, b))      # (copies: writable, contiguous)
    z0, z1 = box_muller(torch.from_numpy(a.view(np.int32)).to(DEV), torch.from_numpy(b.view(np.int32)).to(DEV))
    torch.cuda.synchronize()
    return z0.cpu().numpy(), z1.cpu().numpy()


_SWEEPS = {}


def _sweep(key):
    """A device sweep over all 2^24 fields: "radius" (a = k << 8, b = 0) or an angle sweep at a fixed a (a = key, b = k << 8).  Computed
    once, shared, read-only."""
    if key not in _SWEEPS:
        f = bm.all_fields()
        out = _device(f, np.uint32(0)) if key == "radius" else _device(np.uint32(key), f)
        for x in out:
            x.setflags(write=False)
        _SWEEPS[key] = out
    return _SWEEPS[key]


def _cos_of_zero_turns_is_one():
    """Whether z0 at b = 0 can be read as the radius itself.  The radius is not observable alone, so this is judged from what is: at
    b = 0 the sine term is a zero at every radius, and at each of four radii the four quarter turns give ONE magnitude bitwise (a cosine
    of 0 turns other than 1.0f would have to be matched by the sine of a quarter turn and by both at the half and three-quarter turn).
    Returns (verdict, the largest relative spread of the quarter-turn magnitudes)."""
    z1_zero = not np.any(_sweep("radius")[1])
    spread, same = 0.0, True
    for a in (np.uint32(0), A_MID, A_NEAR_ONE, np.uint32(0x12345600)):
        z0, z1 = _device(a, QUARTERS)
        mags = np.abs(np.float64([z0[0], z1[1], z0[2], z1[3]]))
        same &= bool(np.all(mags == mags[0]))
        spread = max(spread, float(mags.max() / mags.min() - 1.0))
    return z1_zero and same, spread


def test_every_radius():
    z0, z1 = _sweep("radius")
    R = z0.astype(np.float64)
    want = bm.ideal_tables()[0]
    assert not np.isnan(z0).any() and not np.isnan(z1).any(), f"NaN at k = {np.flatnonzero(np.isnan(z0) | np.isnan(z1))[:8]}"
    assert not (z0 < 0).any(), f"a negative radius at k = {np.flatnonzero(z0 < 0)[:8]}"
    assert z0[-1] == 0.0, f"r(u1 = 1) = {z0[-1]!r}"
    exact, spread = _cos_of_zero_turns_is_one()
    tol = bm.RADIUS_RTOL
    if exact:
        _say("z0(a, b = 0) is read as the radius: z1(a, 0) is a zero for every a and the four quarter turns give one magnitude bitwise")
    else:
        # the cosine of 0 turns is not 1.0f (or the sine of 0 turns not 0): its error and the product's rounding join the comparison
        tol = bm.RADIUS_RTOL + spread + bm.EPS
        _say(f"z0(a, b = 0) is NOT bitwise the radius (z1(a, 0) all zero: {not np.any(z1)}; quarter-turn magnitudes differ by up to "
             f"{spread:.3e} relative): the radius is compared under {tol:.3e} instead of {bm.RADIUS_RTOL:.3e}")
    rel = np.abs(R[:-1] / want[:-1] - 1.0)
    k = int(rel.argmax())
    inversions = int(np.count_nonzero(np.diff(R) > 0))
    _say(f"radius: worst relative error {rel[k]:.4e} = {rel[k] / 2.0 ** -23:.3f} x 2^-23 at k = {k} (u1 = {(k + 1) * 2.0 ** -24:.9g}, "
         f"r = {want[k]:.9g}), bound {tol:.4e}; mean signed relative error {np.mean(R[:-1] / want[:-1] - 1.0):+.3e}; "
         f"inversions (device radius increasing with k) at {inversions} of {N - 1} k; max r = {R.max():.9g} (design limit {bm.R_MAX:.9g}); "
         f"r at the three k next to u1 = 1: {z0[-4:-1].tolist()} (fp64 {want[-4:-1].tolist()})")
    assert rel[k] <= tol, (k, rel[k], tol)
    assert R.max() <= bm.R_MAX * (1.0 + tol) and R.max() == R[0]
    # the low 8 bits of either word are ignored, bitwise
    rng = np.random.default_rng(8)
    ks = rng.integers(0, N, size=1 << 16, dtype=np.uint32)
    ks[:4] = (0, 1, N - 2, N - 1)
    low_a = rng.integers(0, 256, size=ks.size, dtype=np.uint32)
    low_b = rng.integers(1, 256, size=ks.size, dtype=np.uint32)
    y0, y1 = _device((ks << np.uint32(8)) | low_a, low_b)
    assert np.array_equal(y0.view(np.uint32), z0[ks].view(np.uint32)) and np.array_equal(y1.view(np.uint32), z1[ks].view(np.uint32))


@pytest.mark.parametrize("a", [np.uint32(0), A_MID, A_NEAR_ONE], ids=["largest radius", "u1 = 0.5", "u1 = 1 - 2^-21"])
def test_every_angle(a):
    z0, z1 = (z.astype(np.float64) for z in _sweep(int(a)))
    r = float(bm.radius(a))
    _, C, S = bm.ideal_tables()
    assert np.isfinite(z0).all() and np.isfinite(z1).all()
    e0, e1 = np.abs(z0 - r * C), np.abs(z1 - r * S)
    ec, es = np.abs(z0 / r - C), np.abs(z1 / r - S)
    kc, ks = int(ec.argmax()), int(es.argmax())
    q = (QUARTERS >> np.uint32(8)).astype(np.int64)
    _say(f"angles at r = {r:.9g} (a = {int(a):#010x}): worst |z0 - fp64| {e0.max():.3e}, |z1 - fp64| {e1.max():.3e} (allowed {bm.Z_ATOL:.0e}); "
         f"worst |cos_dev - cos| {ec[kc]:.3e} at u2 = {kc * 2.0 ** -24:.9g}, |sin_dev - sin| {es[ks]:.3e} at u2 = {ks * 2.0 ** -24:.9g} "
         f"(quotients by the fp64 radius: they carry the radius' own error); mean signed cos error {np.mean(z0 / r - C):+.3e}, "
         f"sin {np.mean(z1 / r - S):+.3e}; max |z0| / r - 1 = {np.abs(z0).max() / r - 1:+.3e}, max |z1| / r - 1 = {np.abs(z1).max() / r - 1:+.3e}; "
         f"quarter turns (z0, z1) / r: {[(float(z0[k] / r), float(z1[k] / r)) for k in q]}")
    assert e0.max() <= bm.Z_ATOL and e1.max() <= bm.Z_ATOL
    bound = r * (1.0 + 2.0 ** -22)
    assert np.abs(z0).max() <= bound and np.abs(z1).max() <= bound


def test_the_exact_moments_of_the_device_distribution():
    R = _sweep("radius")[0].astype(np.float64)
    z0, z1 = _sweep(0)
    C, S = z0.astype(np.float64) / R[0], z1.astype(np.float64) / R[0]
    got = bm.grid_moments(R, C, S)
    ideal = bm.grid_moments(*bm.ideal_tables())
    for k in ("E z0", "E z1", "E z0^2", "E z1^2", "E z0 z1", "E z0^4", "E z1^4", "E r^2", "E r^4", "E cos", "E sin", "E cos sin",
              "E cos^2", "E sin^2", "E cos^4", "E sin^4"):
        _say(f"moments over the 2^24 x 2^24 grid: {k:9s} device {got[k]:+.10e}   ideal fp64 {ideal[k]:+.10e}")
    assert bm.cap_violations(got) == {}


@pytest.mark.parametrize("B,n", [(64, 257), (7, 5)])
def test_the_entry_points_agree(B, n):
    from montecarlopredictivecoding_amd.engine import box_muller, philox_normals
    seed, step, layer, base = 0x1234567890ABCDEF, (1 << 32) - 1, 3, (1 << 32) - 5
    groups = (n + 3) // 4
    raw = philox_normals(seed, step, layer, base, B, 4 * groups, DEV, raw=True)            # [B][groups][4] words
    # ... the words of the NumPy twin, whose u32 chain id wraps inside both batches
    assert np.array_equal(raw.cpu().numpy().view(np.uint32), philox.layer_u32(seed, step, layer, base, B, 4 * groups))
    words = raw.reshape(B * groups * 2, 2)
    z0, z1 = box_muller(words[:, 0].contiguous(), words[:, 1].contiguous())
    got = torch.stack([z0, z1], dim=1).reshape(B, 4 * groups)[:, :n]
    want = philox_normals(seed, step, layer, base, B, n, DEV)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # an empty call launches nothing and returns empty tensors
    e0, e1 = box_muller(words[:0, 0].contiguous(), words[:0, 1].contiguous())
    assert e0.shape == e1.shape == (0,)


# ---- e. the step kernels ---------------------------------------------------------------------------------------------------------------
N_IN, BATCH, T = 3, 37, 6
NETS = {"read-out": ((5, 33, 18), 24), "latent only": ((5, 33), 0)}
FORMS = [None, "ws=0", "ws=2", "ws=2,no_lean=1", "ws=2,spec=0", "ws=3", "ws=4"]
LDS_KERNELS = ("mcpc::mcpc_steps_u_kernel<", "mcpc::mcpc_steps_ws2_kernel<", "mcpc::mcpc_steps_kernel<")


def _ran_the_form(form, pref, step):
    if form is None:
        return any(k in pref for k in LDS_KERNELS) and step.startswith(LDS_KERNELS)
    if form == "ws=0":
        return "mcpc_steps_kernel<" in pref and step.startswith("mcpc::mcpc_steps_kernel<")
    if form == "ws=3":
        return "steps_u_kernel" in pref and step.startswith("mcpc::mcpc_steps_u_kernel<")
    if form == "ws=4":
        return "mcpc_lw_fwd_kernel" in pref and "mcpc_lw_fwd_kernel" in step and "mcpc_lw_bwd_kernel" in step
    ok = "mcpc_steps_ws2_kernel<" in pref and step.startswith("mcpc::mcpc_steps_ws2_kernel<")
    return ok and ("spec=0" not in form or "mcpc_steps_ws2_spec_kernel" not in step)


def _kicks_are_the_reported_normals(net, form, act="relu", seed=77, step_base=5, chain_base=2, slices=(T,)):
    """All weights and biases zero, x0 = 0, lr = 1, noise_var = 0.25: every prediction is 0, x - lr e is exactly 0 and the kick scale is
    exactly 0.5, so the state after step t is 0.5 z of that step, bitwise (as values: the sum 0 + (-0) is +0)."""
    from montecarlopredictivecoding_amd import _lib as L
    from montecarlopredictivecoding_amd.engine import Engine, philox_normals
    sizes, n_out = NETS[net]
    dims = [N_IN] + list(sizes) + ([n_out] if n_out else [])
    eng = Engine(sizes, [{"relu": L.ACT_RELU, "tanh": L.ACT_TANH}[act]] * len(sizes), N_IN, n_out, BATCH, device=DEV, tuning=form)
    try:
        eng.bind_params([torch.zeros(dims[j + 1], dims[j], device=DEV) for j in range(len(dims) - 1)],
                        [torch.zeros(dims[j + 1], device=DEV) for j in range(len(dims) - 1)])
        eng.bind_inputs(None)
        if n_out:
            g = torch.Generator().manual_seed(3)
            eng.bind_target((torch.rand(BATCH, n_out, generator=g) < 0.3).float().to(DEV))
        eng.load_state([torch.zeros(BATCH, n, device=DEV) for n in sizes])
        rec = [torch.full((T, BATCH, n), float("nan"), device=DEV) for n in sizes]
        energies = torch.full((T, L.ENERGY_COLS), float("nan"), dtype=torch.float64, device=DEV)
        t = 0
        for n_steps in slices:
            eng.run(T, t_begin=t, n_steps=n_steps, loss_kind=L.LOSS_BERNOULLI if n_out else L.LOSS_NONE, xopt=L.XOPT_SGD, lr=1.0,
                    noise_mode=L.NOISE_PHILOX, noise_var=0.25, seed=seed, step_base=step_base, chain_base=chain_base,
                    energy_mode=L.ENERGY_ALL, energies_out=energies, rec_begin=0, rec_stride=1, rec_count=T, rec_x=True, rec_x_bufs=rec)
            t += n_steps
        assert t == T
        xs = [torch.empty(BATCH, n, device=DEV) for n in sizes]
        eng.store_state(xs)
        eng.sync_check()
        pref, step = eng.query()["step_kernel"], eng.last_step_kernel()
    finally:
        eng.close()
    assert _ran_the_form(form, pref, step), (form, pref, step)
    en = energies.cpu().numpy()
    for l, n in enumerate(sizes):
        states = np.concatenate([rec[l].cpu().numpy(), xs[l].cpu().numpy()[None]])             # x_0 .. x_T
        assert not states[0].any(), (form, l)
        for s in range(T):
            want = philox_normals(seed, (step_base + s) & 0xFFFFFFFFFFFFFFFF, l, chain_base, BATCH, n, DEV).cpu().numpy() * np.float32(0.5)
            assert np.array_equal(states[s + 1], want), \
                f"{form or 'default'} ({step}), layer {l}, step {s}: {np.count_nonzero(states[s + 1] != want)} of {want.size} kicks differ"
        # the padded units of a layer (widths 5, 33 and 18 are no multiple of a 4-unit group or a 16-unit tile) stay zero: the layer
        # energy is that of the n recorded units (fp32 partial sums of at most 37 x 33 squares: 1e-5; one kicked padded unit of one
        # chain would add 1e-3 of it on average)
        np.testing.assert_allclose(en[:, 1 + l], 0.5 * (states[:T].astype(np.float64) ** 2).sum((1, 2)), rtol=1e-5, atol=1e-12)
    return step


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("form", FORMS, ids=[f or "default" for f in FORMS])
def test_every_step_kernel_form_applies_the_reported_normals(form, net):
    _say(f"step kernels: {form or 'default'}, {net}: ran {_kicks_are_the_reported_normals(net, form)!r}")


def test_a_tanh_net_applies_the_reported_normals():
    _kicks_are_the_reported_normals("read-out", None, act="tanh")


EDGES = {"step counter across 2^32": dict(step_base=(1 << 32) - 3),
         "chain id wraps inside the batch": dict(chain_base=(1 << 32) - 20),
         "64-bit seed": dict(seed=0xFEDCBA9876543210),
         "slices of 1, 2 and 3 steps": dict(slices=(1, 2, 3))}


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("form", [None, "ws=0"], ids=["default", "ws=0"])
def test_counter_edges_inside_the_step_kernels(form, edge):
    _kicks_are_the_reported_normals("read-out", form, **EDGES[edge])

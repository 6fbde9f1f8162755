"""The cases of tests/scale_swing_cases.py on the CPU: every schedule has its teeth on the oracle's fp64 trajectory (a schedule that lost them
fails here, before a GPU is involved), the plan cuts the read-out into more chunks than its ring has slots, and the oracle's own fp32
evaluation keeps a margin of a half under every bound the GPU tests assert."""
import numpy as np
import pytest

from tests import scale_swing_cases as sc

HALF = 0.5


def _log2(values):
    return [round(float(np.log2(v)), 2) for v in values]


# ---- Part A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("readout", [True, False], ids=["readout", "no_readout"])
@pytest.mark.parametrize("act", sc.A_ACTS)
def test_the_kick_schedule_has_its_teeth_on_the_fp64_oracle(act, readout):
    states, _ = sc.a_oracle(act, readout)
    lo, hi, rise, fall = sc.a_teeth(states, act)
    print(f"[scale swings A, fp64 oracle] {act}, read-out {readout}: row maxima 2^{_log2([lo, hi])}, per tile, step and layer a rise of at "
          f"least 2^{_log2([rise])[0]} and a fall of at least 2^{_log2([fall])[0]}")
    # every state of the cycle in every tile at every step
    for t in range(sc.A_T + 1):
        for c0 in (0, 16, 32):
            assert {sc.a_state(t, c) for c in range(c0, min(c0 + 16, sc.B))} == set(sc.CYCLE)


def test_the_round_schedule_case_has_its_teeth_and_its_batch_comes_from_the_plan():
    from tests import plan_util
    batch = sc.round_batch(256)
    assert batch % 16 == 0 and batch > 16 * 256
    assert plan_util.plan(sc.SIZES, sc.N_OUT, batch, None, n_cu=256, n_in=sc.N_IN)["rounds"]["on"]
    assert not plan_util.plan(sc.SIZES, sc.N_OUT, batch - 16, None, n_cu=256, n_in=sc.N_IN)["rounds"]["on"]
    states, _ = sc.a_oracle("relu", True, batch)
    sc.a_teeth(states, "relu")


def test_a_constant_scale_chain_changes_nobody_else_on_the_oracle():
    """Assertion 4 on the oracle: the kicks of every other chain are the same arrays, so are their trajectories."""
    base, flat = sc.a_kicks(), sc.a_kicks(flat=sc.A_FLAT)
    others = np.arange(sc.B) != sc.A_FLAT
    for a, f in zip(base, flat):
        assert np.array_equal(a[:, others], f[:, others]) and not np.array_equal(a[:, sc.A_FLAT], f[:, sc.A_FLAT])
        assert np.abs(f[:, sc.A_FLAT]).max() < 1.0 and np.abs(f[:, sc.A_FLAT]).min() >= 0.5


@pytest.mark.parametrize("readout", [True, False], ids=["readout", "no_readout"])
@pytest.mark.parametrize("act", sc.A_ACTS)
def test_the_fp32_oracle_keeps_half_of_the_bounds_of_part_a(act, readout):
    W, b, _, inputs, target = sc.a_data(act, readout)
    states, _ = sc.a_oracle(act, readout, dtype="float32")
    kicks = sc.a_kicks()
    worst = sc.steps_vs_fp64(sc.a_case(act, readout), W, b, inputs, target, states, lambda t: [k[t] for k in kicks])
    print(f"[scale swings A, fp32 oracle] {act}, read-out {readout}: a step is within {worst:.2e} of sum |terms| (bound {sc.STEP_RTOL:.0e})")
    assert 0 < worst <= HALF * sc.STEP_RTOL
    if readout:
        x_last = states[-1][:-1]
        got = sc.outputs_vs_fp64(W, b, act, x_last, sc.outputs_fp32(W, b, act, x_last))
        bound = sc.out_bound(sc.SIZES[-1])
        print(f"[scale swings A, fp32 oracle] {act}: a read-out row is within {got:.2e} of sum |terms| (bound {bound:.2e})")
        assert 0 < got <= HALF * bound


# ---- Part B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", sc.B_REGIMES)
def test_the_dynamics_have_their_teeth_on_the_fp64_oracle(regime):
    lo, hi, move = sc.b_teeth(sc.b_oracle(regime), regime)
    print(f"[scale swings B, fp64 oracle] {regime}: row maxima 2^{_log2([lo, hi])}, smallest move asserted 2^{_log2([move])[0]}")
    # every tile holds the whole range of initial scales
    e = sc.b_chain_exponents()
    for c0 in (0, 16, 32):
        assert e[c0:c0 + 16].min() <= -7 and e[c0:c0 + 16].max() >= 7
    assert e.min() == -12 and e.max() == 12


@pytest.mark.parametrize("regime", sc.B_REGIMES)
def test_the_fp32_oracle_keeps_half_of_the_bounds_of_part_b(regime):
    W, b, _, _, target = sc.b_data(regime)
    states = sc.b_oracle(regime, dtype="float32")
    sc.b_teeth(states, regime)
    if regime == "adam":
        worst = sc.adam_steps_vs_fp64(sc.b_case(regime), W, b, target, states)
        print(f"[scale swings B, fp32 oracle] adam: a step uses {worst:.3f} of its bound")
        assert 0 < worst <= HALF
    else:
        worst = sc.steps_vs_fp64(sc.b_case(regime), W, b, None, target, states, sc.b_kicks_of(regime))
        print(f"[scale swings B, fp32 oracle] {regime}: a step is within {worst:.2e} of sum |terms| (bound {sc.STEP_RTOL:.0e})")
        assert 0 < worst <= HALF * sc.STEP_RTOL


def test_the_decaying_readout_is_saturated_exactly():
    """b_out = +-110: the fp32 sigmoid is exactly the target, so no back-projected read-out error holds the last layer's rows up."""
    W, b, X0, _, target = sc.b_data("decay")
    o = sc.outputs_fp32(W, b, "relu", X0[-1])
    with np.errstate(over="ignore"):
        assert np.array_equal((np.float32(1.0) / (np.float32(1.0) + np.exp(-o))).astype(np.float32), target)
    assert min(float(w.min()) for w in W[:3]) > 0 and min(float(x.min()) for x in X0) > 0


# ---- Part C ---------------------------------------------------------------------------------------------------------------------------------
def test_the_plan_cuts_the_readout_into_more_chunks_than_the_ring_has_slots():
    from tests import plan_util
    p = plan_util.plan(sc.SIZES, sc.N_OUT, sc.B, "ws=2", n_in=sc.N_IN)
    chunk, ring = p["main"]["chunk"], p["main"]["ring"]
    assert chunk > 0 and ring > 0
    assert -(-(p["out_pad"] // 16) // chunk) > ring, (p["out_pad"], chunk, ring)
    units, n, ring_ = sc.c_chunks()
    assert (units, ring_) == (16 * chunk, ring) and n >= 4          # (Part A wants four chunks at least)
    # 784 is the smallest of the read-outs the project uses elsewhere that does (tests/test_gpu_flush.py, wide_cases.py)
    for n_out in (100, 264, 520):
        q = plan_util.plan(sc.SIZES, n_out, sc.B, "ws=2", n_in=sc.N_IN)
        assert -(-(q["out_pad"] // 16) // q["main"]["chunk"]) <= q["main"]["ring"], n_out


@pytest.mark.parametrize("order", sc.C_ORDERS)
def test_the_chunk_case_is_block_sparse_and_the_fp32_oracle_keeps_half_of_its_bound(order):
    W, b, X0, _, target, unit_chunk, latent_chunk, ex = sc.c_data(order)
    _, n, _ = sc.c_chunks()
    assert sorted(ex) == sorted(sc.c_exponents("ascending", n)) and np.all(np.abs(np.diff(sorted(ex))) == sc.C_STEP)
    assert max(abs(e) for e in ex) <= 40
    assert ex.index(max(ex)) == {"ascending": n - 1, "descending": 0, "peak in the middle": n // 2}[order]
    # every unit of the last latent layer meets the read-out units of one chunk only, and every chunk is met
    for j in range(sc.SIZES[-1]):
        assert set(unit_chunk[W[3][:, j] != 0]) == {latent_chunk[j]}
    assert set(latent_chunk) == set(range(n))
    want, terms, bound = sc.c_reference(order)
    got = (-target) @ W[3]                                     # the oracle's back-projection of e_o = -y, in fp32
    assert got.dtype == np.float32 and np.isfinite(got).all() and (terms > 0).all()
    frac = np.abs(got.astype(np.float64) - want) / terms / bound
    sharp = bound < 1e-5                                       # the chunk that holds the maximum
    print(f"[scale swings C, fp32 oracle] {order}: error / bound {frac.max():.3f}; in the chunk of the maximum {frac[sharp].max():.3f}")
    assert sharp.any() and frac.max() <= HALF and frac[sharp].max() > 0


@pytest.mark.parametrize("order", sc.C2_ORDERS)
def test_the_two_step_cases_move_the_chunks_as_they_say(order):
    states, outs = sc.c2_oracle(order)
    s = sc.c2_teeth(outs, order)
    print(f"[scale swings C, fp64 oracle] two steps, {order}: chunk scales of e_o 2^{np.round(s[0], 1).tolist()} then 2^{np.round(s[1], 1).tolist()}")
    assert max(float(np.abs(x).max()) for x in states) <= 2.0 ** 40 and float(np.abs(outs).max()) <= 2.0 ** 40
    W, b, _, _, target = sc.c2_data(order)
    states32, outs32 = sc.c2_oracle(order, dtype="float32")
    sc.c2_teeth(outs32, order)
    worst = sc.steps_vs_fp64(sc.c_case(), W, b, None, target, states32, lambda t: None)
    assert 0 < worst <= HALF * sc.STEP_RTOL, worst

"""CPU checks of tests/special_value_cases.py: every case the GPU file uses is a parity case at the bounds it asserts, and the premise
of its confinement assertion -- a special chain changes no other chain -- holds for the oracle itself.

In the manner of tests/test_wide_cases.py: the oracle's own fp32 run stays within A FIFTH of each bound the GPU test holds the engine
to (special chain: states and records 1e-6 max(10, max |x|); its per-chain energies the bound of chain_energy_cases.oracle_rows;
energy table rtol 1e-6; gradient bucket rtol 2e-4 + 2e-5 max |want|).  A case that misses this is replaced, never given a wider bound."""
import numpy as np
import pytest

from tests import special_value_cases as sv
from tests import wide_cases as wc

FINITE_CASES = [(n, c, k, ch) for n in sorted(sv.NETS) for c in sorted(sv.COMBOS) for k in sv.kinds(c) if k in sv.FINITE for ch in sv.CHAINS]
ALL_CASES = [(n, c, k, ch) for n in sorted(sv.NETS) for c in sorted(sv.COMBOS) for k in sv.kinds(c) for ch in sv.CHAINS]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("net,combo,kind,chain", FINITE_CASES)
def test_the_oracle_in_fp32_uses_a_fifth_of_each_bound(net, combo, kind, chain):
    a, b = sv.oracle(net, combo, kind, chain, "float32"), sv.oracle(net, combo, kind, chain, "float64")
    # the special chain's states and records
    bound = sv.state_bound(net, combo, kind, chain)
    dx = max(float(np.abs(x.astype(np.float64) - y).max()) for ra, rb in zip(sv.chain_states(a, chain), sv.chain_states(b, chain))
             for x, y in zip(ra, rb))
    # the energy table
    assert np.isfinite(b.overall).all() and np.isfinite(a.overall).all()
    de = max(float(np.max(np.abs(p - q) / np.abs(q))) for p, q in ((a.overall, b.overall), (a.loss, b.loss), (a.layer_energy, b.layer_energy)))
    # the bucket
    ga, gb = wc.bucket(a), wc.bucket(b)
    dg = float(np.max(np.abs(ga - gb) / (2e-4 * np.abs(gb) + 2e-5 * np.abs(gb).max())))
    # the special chain's per-chain energies, on the fp32 run's own records
    xs = [np.stack([a.rec_xs[t][l][chain:chain + 1] for t in range(sv.T)]) for l in range(len(sv.NETS[net]["sizes"]))]
    want, rb = sv.chain_rows(net, combo, chain, xs)
    got, _ = sv.chain_rows(net, combo, chain, xs, dtype=np.float32)
    dr = float(np.max(np.abs(got - want) / rb))
    print("%s %s %s chain %d: states %.2e of %.2e (scale %.3g)  energies %.2e  bucket %.3f  chain rows %.3f of their bounds"
          % (net, combo, kind, chain, dx, bound, sv.chain_scale(net, combo, kind, chain), de, dg, dr))
    assert dx <= bound / 5 and de <= 1e-6 / 5 and dg <= 1 / 5 and dr <= 1 / 5, (dx, bound, de, dg, dr)


@pytest.mark.parametrize("net,combo,kind,chain", ALL_CASES)
def test_the_oracles_other_chains_do_not_see_the_special_one(net, combo, kind, chain):
    """fp32, as the engine computes: every state and record of every other chain is bitwise the baseline's."""
    a, base = sv.oracle(net, combo, kind, chain, "float32"), sv.oracle(net, combo, None, 0, "float32")
    others = np.arange(sv.B) != chain
    for xa, xb in zip(a.xs, base.xs):
        assert np.array_equal(xa[others], xb[others])
        assert not _same(xa[chain], xb[chain])
    for t in range(sv.T):
        for xa, xb in zip(a.rec_xs[t], base.rec_xs[t]):
            assert np.array_equal(xa[others], xb[others])
        assert np.array_equal(a.rec_out[t][others], base.rec_out[t][others])


@pytest.mark.parametrize("net", sorted(sv.NETS))
def test_the_special_rows_are_what_they_are_called(net):
    combo = "relu_bernoulli"
    _, _, X0, _, _ = sv.data(net, combo)
    for chain in sv.CHAINS:
        # dead: f(x) = 0 on every one of the four steps (lr 0.05 and noise_var 2 do not carry x from -5 to 0)
        for dtype in ("float32", "float64"):
            r = sv.oracle(net, combo, "dead", chain, dtype)
            assert max(float(x.max()) for rows in sv.chain_states(r, chain)[:sv.T] for x in rows) < 0
        for x in sv.special_x0(X0, "denormal", chain):
            row = np.abs(x[chain])
            assert row.max() > 0 and (row.view(np.uint32) >> 23).max() == 0          # exponent field 0
        for x in sv.special_x0(X0, "huge", chain):
            assert 2.0 ** 30 < np.abs(x[chain]).max() < 2.0 ** 41
        for kind in sv.NONFINITE:
            for x, x0 in zip(sv.special_x0(X0, kind, chain), X0):
                assert not np.isfinite(x[chain, 0]) and np.array_equal(x[chain, 1:], x0[chain, 1:])
        for x, x0 in zip(sv.special_x0(X0, "nan", chain), X0):
            others = np.arange(sv.B) != chain
            assert np.array_equal(x[others], x0[others])
    # the energy of a huge chain stays far inside fp32
    assert sv.oracle(net, combo, "huge", 21).overall.max() < 1e30


def test_the_table_is_what_the_gpu_file_needs():
    assert sv.B == 40 and sv.T == 4 and sv.CHAINS == (21, 16, 39)
    assert (sv.NETS["short"]["sizes"], sv.NETS["short"]["n_out"]) == ([33, 48, 17], 40)
    assert (sv.NETS["long"]["sizes"], sv.NETS["long"]["n_out"]) == ([33, 200, 96], 112)
    assert sv.kinds("relu_bernoulli") == ("dead", "huge", "denormal", "+inf", "-inf", "nan")
    assert sv.kinds("tanh_gaussian") == ("huge", "denormal", "+inf", "-inf", "nan")
    for net in sv.NETS:
        for combo in sv.COMBOS:
            c = sv.case(net, combo)
            assert c["B"] == 40 and c["T"] == 4 and not c["inputs_zero"]
            assert sv.case(net, combo, readout=False)["n_out"] == 0

"""The host planner (csrc/mcpc_plan.h: plan_engine) through mcpc_debug_plan -- no GPU: the plans DESIGN.md documents, the fallbacks of
mcpc_create, and what every LDS plan, step table and round schedule must satisfy, over a seeded sweep of networks."""
import random

import pytest

from tests.plan_util import entries, plan

LDS_LIMIT = 163840
ENOMEM = -3
PH_FWD, PH_HEADF, PH_HEADB, PH_BWD = 0, 1, 2, 3
CFG_M = dict(sizes=[30, 256, 256], n_out=784)


def _error(**kw):
    from montecarlopredictivecoding_amd import _lib
    with pytest.raises(_lib.MCPCError) as exc:
        plan(**kw)
    return exc.value.code, str(exc.value)


# ---- known plans (DESIGN.md sections 4 and 5) ------------------------------------------------------------------------------------------------
def test_headline_plan_of_the_benchmark_net():
    p = plan(batch=6000, **CFG_M)
    m = p["main"]
    assert p["form"] == "in-place" and p["Bpad"] == 6016 and p["workgroups"] == 375 and p["chains_per_wg"] == 16
    assert m["lds_bytes"] == 158976 and m["xl"] == 1
    assert (m["ring"], m["chunk"], m["overlay"]) == (3, 14, 0)          # three chunks of 14 tiles, apart from the E_l
    assert m["n_phases"] == 15 and len(m["table"]) == 15
    assert (p["rounds"]["on"], p["rounds"]["k"], p["rounds"]["m"]) == (1, 3, 2)
    assert [len(rows) for rows in p["rounds"]["launches"]] == [250, 250, 250]
    assert p["kernel"] == "mcpc::mcpc_steps_ws2_kernel<1, true> (round schedule: k=3 launches per cycle, every 16-chain unit in m=2 of them)"
    assert p["slots"] == 384 and p["half_slots"] == 128 and p["spill_tm"] == [0, 1, 1, 1]


def test_unified_plan_of_the_benchmark_net_leaves_the_target_words_in_global_memory():
    u = plan(batch=6000, **CFG_M)["unified"]
    assert (u["ok"], u["on"], u["prefer"]) == (1, 1, 0)                 # held for zero-loss calls, not preferred at this width
    assert u["plan"]["lds_bytes"] == 163776 and u["plan"]["lds_yw"] == -1
    assert "yw" not in [r[0] for r in u["plan"]["regions"]]
    assert u["plan"]["rows"] == 8


def test_the_reference_net_prefers_the_unified_kernel():
    p = plan(sizes=[20, 128, 128], n_out=784, batch=256)
    assert p["unified"]["prefer"] == 1 and p["kernel"] == "mcpc::mcpc_steps_u_kernel<false>"
    assert p["unified"]["plan"]["lds_yw"] >= 0 and p["rounds"]["on"] == 0


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------------------------
def test_a_hidden_width_no_lds_plan_holds():
    code, msg = _error(sizes=[30, 1024, 1024], n_out=0, batch=100)
    assert code == ENOMEM and "latent widths too large for the fused kernel" in msg
    p = plan(sizes=[30, 1024, 1024], n_out=0, batch=100, tuning="wide=1")
    assert p["form"] == "layer-wise" and p["Bpad"] == 128 and p["Bpad"] % 64 == 0
    assert p["kernel"] == "mcpc::mcpc_lw_fwd_kernel + mcpc::mcpc_lw_bwd_kernel" and p["main"]["table"] == []
    assert p["lw"]["n_fwd"] + p["lw"]["n_bwd"] == len(p["lw"]["jobs"]) and p["workgroups"] == 2 * p["lw"]["n_fwd"]


def test_a_last_latent_layer_too_wide_for_the_read_out():
    code, msg = _error(sizes=[30, 64, 272], n_out=10, batch=100)
    assert code == ENOMEM and "last latent layer wider than 256 units is not supported by the fused read-out" in msg
    p = plan(sizes=[30, 64, 272], n_out=10, batch=100, tuning="wide=1")
    assert p["form"] == "layer-wise" and p["Bpad"] == 128


def test_ws4_refuses_the_knobs_of_the_lds_kernels():
    code, msg = _error(sizes=[30, 64], n_out=10, batch=100, tuning="ws=4,no_xl=1")
    assert code == -1 and "tuning ws=4 (layer-wise kernels) together with no_xl" in msg
    assert plan(sizes=[30, 64], n_out=10, batch=100, tuning="ws=4")["form"] == "layer-wise"


def test_ws3_without_a_unified_plan_is_refused():
    code, msg = _error(sizes=[30, 256, 256], n_out=2000, batch=100, tuning="ws=3")
    assert code == ENOMEM and "tuning ws=3: the unified-wave kernel's LDS plan does not fit this network" in msg
    assert plan(sizes=[30, 256, 256], n_out=2000, batch=100)["unified"]["on"] == 0        # ... which runs in place without the knob
    assert plan(sizes=[30, 256, 256], n_out=2000, batch=100, tuning="ws=3,wide=1")["form"] == "layer-wise"


# ---- invariants over a seeded sweep ---------------------------------------------------------------------------------------------------------
def _sweep(seed=20240607, count=300):
    """1-6 latent layers of 1-600 units (log-uniform: LDS plans exist for most), with and without read-out, batch 1-9000."""
    rng = random.Random(seed)
    for _ in range(count):
        sizes = [min(600, int(round(600 ** rng.random()))) for _ in range(rng.randint(1, 6))]
        n_out = rng.choice([0, 0, rng.randint(1, 1200)])
        knobs = ["ws=%d" % ws for ws in [rng.choice([0, 2, 3])] if rng.random() < 0.5]
        knobs += [k for k in ("no_xl", "overlay16") if rng.random() < 0.25]
        yield dict(sizes=sizes, n_out=n_out, batch=rng.randint(1, 9000), tuning=",".join(knobs) or None, n_cu=rng.choice([64, 256, 304]))


def _check_lds(sp):
    assert 0 < sp["lds_bytes"] <= LDS_LIMIT
    regions = [r for r in sp["regions"] if r[3] > 0]
    for name, layer, off, floats in regions:
        assert off >= 0 and 4 * (off + floats) <= sp["lds_bytes"], (name, layer)
    for i, a in enumerate(regions):
        for b in regions[i + 1:]:
            if a[2] < b[2] + b[3] and b[2] < a[2] + a[3]:
                assert sp["overlay"] == 1 and {a[0], b[0]} == {"ring", "e"}, (a, b)


def _check_cover(rows, sizes, n_out, strided):
    """Every unit tile of every layer once by the FWD entries and once by the BWD entries, every read-out tile once by HEADF."""
    seen = {}
    for k in rows:
        if k["type"] in (PH_FWD, PH_HEADF, PH_BWD):
            for i in range(k["ntiles"]):
                key = (k["type"], k["layer"], k["tile0"] + (k["rot"] * i if strided else i))
                seen[key] = seen.get(key, 0) + 1
    tiles = lambda n: (n + 15) // 16
    want = {(t, l, u) for t in (PH_FWD, PH_BWD) for l, n in enumerate(sizes) for u in range(tiles(n))}
    want |= {(PH_HEADF, len(sizes) - 1, u) for u in range(tiles(n_out))}
    assert set(seen) == want and set(seen.values()) == {1}, sorted(set(seen) ^ want)[:5]


def test_every_plan_of_the_sweep_is_sound():
    from montecarlopredictivecoding_amd import _lib
    rejected, forms, n_unified, n_rounds = 0, set(), 0, 0
    nets = list(_sweep())
    for net in nets:
        try:
            p = plan(**net)
        except _lib.MCPCError as exc:
            assert exc.code == ENOMEM, (net, str(exc))          # never another refusal, and no net is skipped
            rejected += 1
            continue
        forms.add(p["form"])
        assert p["form"] in ("in-place", "barrier") and p["Bpad"] % 16 == 0 and p["Bpad"] >= net["batch"], net
        m = p["main"]
        _check_lds(m)
        rows = entries(m)
        assert len(rows) == m["n_phases"] > 0
        if p["form"] == "in-place":
            # (in the unified table these fields carry fragment offsets, in the barrier table nothing)
            for k in rows:
                assert all(-1 <= k[f] < len(rows) for f in ("dep_e", "dep_g", "dep_se", "next_g")), (net, k)
            assert -1 <= m["g_first"] < len(rows)
        _check_cover(rows, net["sizes"], net["n_out"], strided=False)
        if p["unified"]["on"]:
            n_unified += 1
            u = p["unified"]["plan"]
            _check_lds(u)
            assert u["rows"] == 8 and len(u["table"]) == 8 * u["n_phases"]
            _check_cover(entries(u), net["sizes"], net["n_out"], strided=True)
        r = p["rounds"]
        if r["on"]:
            n_rounds += 1
            assert p["form"] == "in-place" and p["workgroups"] > net["n_cu"]
            assert all(0 < len(rows_) <= net["n_cu"] for rows_ in r["launches"]) and len(r["launches"]) == r["k"]
            assert sorted(u_ for rows_ in r["launches"] for u_, _ in rows_) == sorted(list(range(p["workgroups"])) * r["m"])
    print("sweep of %d nets: %d rejected (MCPC_ENOMEM), %d with a unified plan, %d on the round schedule" % (len(nets), rejected, n_unified, n_rounds))
    assert rejected <= len(nets) // 4, rejected
    assert forms == {"in-place", "barrier"} and n_unified >= 30 and n_rounds >= 30
